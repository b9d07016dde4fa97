"""Input side of the hot path: decoded uint8 frames are normalised ON THE DEVICE, and host batches
are staged through pinned memory on a copy stream one batch ahead of the compute.

The reference normalises on the host (`EVESequencesBase.preprocess_frames` / `preprocess_screen_frames`,
/root/reference/src/datasources/eve_sequences.py:196-211) and moves float tensors with `.to(device, non_blocking=True)`
from pageable memory (src/core/training.py:257-261): 377 MB per 960-frame step for the eye patches alone.  Shipping the
uint8 frames is 4x less PCIe traffic, and the float values produced here are bit-identical to numpy's.

  preprocess_frames(u8)          [..., H, W, C] uint8 (device) -> [..., C, H, W] float32 in [-1, 1]
  preprocess_screen_frames(u8)   same, [0, 1]
  preprocess_screen_frames(u8, size=(H, W))
                                 [..., IH, IW, 3|4] uint8 of any size >= (H, W), e.g. a 1920 x 1080 capture -> [..., 3, H, W]
                                 float32 in [0, 1] by exact area averaging (RefineNet passes its screen_size for uint8 screens)
  preprocess_screen_frames(u8, size=(H, W), bgr=True)
                                 the same from a BGR(A) capture: the planes come out in RGB order, no swapped copy is made
  preprocess_screen_frames(u8, size=(H, W), format='nv12', matrix='bt601')
                                 the same from a decoder's or capture path's NV12 / I420 [..., IH*3/2, IW] or YUYV [..., IH, IW, 2]
                                 surface: converted pixel by pixel as it is read, then averaged -- the keys `screen_frame_nv12`,
                                 `screen_frame_i420`, `screen_frame_yuyv` in place of `screen_frame`
  warp_eye_patches(u8, warps)    whole camera frames [..., IH, IW, 3|4] uint8 and per-frame homographies [..., 3, 3] float32
                                 (patch pixel -> camera pixel) -> one eye's patches [..., 3, H, W] float32 in [-1, 1], cut
                                 bilinearly on the device (EyeNet / EVE / EVEStream take `camera_frame` + `<side>_eye_warp`)
  warp_eye_patches(u8, warps, format='nv12', matrix='bt601')
                                 the same from frames as cameras and decoders deliver them: format 'bgr' [..., IH, IW, 3|4], 'nv12' /
                                 'i420' [..., IH*3/2, IW], 'yuyv' [..., IH, IW, 2]; only the taps read are converted, by a bit-exact
                                 integer matrix ('bt601', 'bt709' limited range, 'jfif' full range) -- the keys `camera_frame_bgr`,
                                 `camera_frame_nv12`, `camera_frame_i420`, `camera_frame_yuyv` in place of `camera_frame`
  SurfaceLayout(format, width, height, pitch=, coded_height=, x0=, y0=, plane_offsets=)
                                 how a decoder's or capture API's surface lies in memory (pitched rows, coded rows, a crop; NV21,
                                 YV12, UYVY, P010, pitched BGRA, ...): warp_eye_patches(..., layout=) and preprocess_screen_frames(...,
                                 layout=) read the visible region where it lies -- the keys `camera_surface` / `screen_surface` with
                                 model.eye_net.camera_layout / model.refine_net.screen_layout
  camera_lens(K, dist)           a camera matrix [..., 3, 3] and 4, 5 or 8 OpenCV distortion coefficients -> the float32 [..., 12]
                                 rows that warp_eye_patches(..., lens=) and the `camera_lens` key take for RAW (distorted) frames
  eye_pose(K, rvec, tvec, eyes, focal_norm, distance_norm)
                                 a face tracker's cv2.solvePnP result -> the float32 [..., 18] rows of the `eye_pose` key (EyeNet /
                                 EVE / EVEStream take `camera_frame` + `eye_pose` and derive the warps, R, o, h and head_R on the device)
  normalize_eyes(pose)           those rows -> the derived tensors themselves (head_R, <side>_o, _R, _eye_warp, _h, pose_valid)
  face_rig(K, model, eyes, focal_norm, distance_norm)
                                 a camera and a head model -> the float32 [..., 12 + 3L] rows of the `face_rig` key (EyeNet / EVE /
                                 EVEStream take `camera_frame` + `face_landmarks` + `face_rig` and solve the head pose on the device)
  solve_head_pose(landmarks, rig) 2-D landmarks -> head_R, head_t, reproj_rms, valid (in place of cv2.solvePnP per frame); lens= takes
                                 landmarks of the RAW frame, huber_px= a Huber loss against landmarks that are confidently wrong
  undistort_points(points, lens) raw-frame pixels -> pixels of the undistorted image (in place of cv2.undistortPoints)
  EyeNet.forward_sequence / RefineNet.forward_sequence / EVE accept the uint8 tensors directly (eye patches go straight
  into the stem kernel's packed bf16 layout, no float tensor is ever materialised).
  DevicePrefetcher(iterable)     pinned double-buffered H2D on a side stream
"""
import numpy as np
import torch

from .kernels import default_kernels

EYE_SCALE, EYE_SHIFT = 2.0 / 255.0, -1.0        # eve_sequences.py:200-201
SCREEN_SCALE = 1.0 / 255.0                      # eve_sequences.py:209


def _fold(frames):
    if frames.dtype != torch.uint8 or frames.dim() < 4:
        raise TypeError('expected uint8 frames shaped [..., H, W, C], got %s %s' % (frames.dtype, tuple(frames.shape)))
    lead = tuple(frames.shape[:-3])
    return frames.reshape((-1,) + tuple(frames.shape[-3:])).contiguous(), lead


# SurfaceLayout formats -> (kind 'rgb' | 'yuv', bytes per pixel of the first plane, planes after it, xshift, yshift)
SURFACE_FORMATS = {'rgb': ('rgb', 3, 0, 0, 0), 'rgba': ('rgb', 4, 0, 0, 0), 'bgr': ('rgb', 3, 0, 0, 0), 'bgra': ('rgb', 4, 0, 0, 0),
                   'nv12': ('yuv', 1, 1, 1, 1), 'nv21': ('yuv', 1, 1, 1, 1), 'i420': ('yuv', 1, 2, 1, 1), 'yv12': ('yuv', 1, 2, 1, 1),
                   'yuyv': ('yuv', 2, 0, 1, 0), 'uyvy': ('yuv', 2, 0, 1, 0), 'p010': ('yuv', 2, 1, 1, 1)}


class SurfaceLayout(object):
    """How a decoder's or capture API's surface lies in memory: the descriptor of include/eve_hip.h eve_surface, computed from what
    such an API reports.  A frame is one byte range; component c of visible pixel (x, y) is the byte
    offset[c] + (y >> ys) * pitch[c] + (x >> xs) * step[c] of it -- nothing else is read, so padding, coded rows below the picture
    and a fourth channel never reach a result.
      format         'rgb' | 'rgba' | 'bgr' | 'bgra' (packed, 3 or 4 bytes per pixel), 'nv12' | 'nv21' (luma plane, then one plane of
                     interleaved U, V | V, U), 'i420' | 'yv12' (luma, then the U, V | V, U planes at half the pitch), 'yuyv' | 'uyvy'
                     (Y U Y V | U Y V Y per pixel pair), 'p010' (NV12's shape in 16-bit little-endian words, read as their high
                     byte: the sample >> 8, a truncation to 8 bits)
      width, height  the visible region in pixels
      pitch          bytes from one row of the first plane to the next; None: the tight row, (x0 + width) pixels
      coded_height   rows each plane was allocated for (the chroma planes of the 4:2:0 formats: half of it); None: height + y0
      x0, y0         the visible region's top-left pixel inside the surface: a crop, or a window of a captured desktop.  Odd along
                     a subsampled axis is a ValueError: the chroma phase would shift
      plane_offsets  None, or the byte where each plane after the first begins (one value for nv12 / nv21 / p010, two for i420 /
                     yv12, in memory order), for allocators that align planes; None: each plane follows the one before
    frame_bytes is what one frame occupies, and frame_stride the same: the tensor handed over with the layout is a contiguous
    uint8 [..., rows, pitch] or [..., frame_bytes] whose trailing dimensions multiply to it.  Instances compare and hash by value."""

    def __init__(self, format, width, height, pitch=None, coded_height=None, x0=0, y0=0, plane_offsets=None):
        if format not in SURFACE_FORMATS:
            raise ValueError('SurfaceLayout: format must be one of %s, got %r' % (', '.join(SURFACE_FORMATS), format))
        kind, bpp, nplanes, xs, ys = SURFACE_FORMATS[format]
        ints = dict(width=width, height=height, x0=x0, y0=y0)
        if pitch is not None:
            ints['pitch'] = pitch
        if coded_height is not None:
            ints['coded_height'] = coded_height
        for name, v in ints.items():
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
                raise ValueError('SurfaceLayout: %s must be an integer, got %r' % (name, v))
        width, height, x0, y0 = int(width), int(height), int(x0), int(y0)
        if width < 1 or height < 1 or x0 < 0 or y0 < 0:
            raise ValueError('SurfaceLayout: width and height must be >= 1 and x0, y0 >= 0, got %d x %d at (%d, %d)' % (width, height, x0, y0))
        if (xs and (x0 % 2 or width % 2)) or (ys and (y0 % 2 or height % 2)):
            raise ValueError('SurfaceLayout: %s subsamples chroma: the crop origin and size must be even along %s, got %d x %d at (%d, %d) '
                             '(an odd origin would shift the chroma phase)' % (format, 'x and y' if ys else 'x', width, height, x0, y0))
        tight = (x0 + width) * bpp
        pitch = tight if pitch is None else int(pitch)
        coded = y0 + height if coded_height is None else int(coded_height)
        if pitch < tight:
            raise ValueError('SurfaceLayout: pitch %d is shorter than the %d bytes of x0 + width = %d pixels' % (pitch, tight, x0 + width))
        if pitch >= 2 ** 31:
            raise ValueError('SurfaceLayout: pitch must fit 31 bits, got %d' % pitch)
        if coded < y0 + height:
            raise ValueError('SurfaceLayout: coded_height %d is less than y0 + height = %d' % (coded, y0 + height))
        if nplanes == 2 and pitch % 2:
            raise ValueError('SurfaceLayout: %s chroma planes have half the pitch: pitch must be even, got %d' % (format, pitch))
        cpitch = pitch // 2 if nplanes == 2 else pitch                    # of the planes after the first
        crows = (coded + 1) // 2
        if plane_offsets is None:
            starts = [pitch * coded + i * cpitch * crows for i in range(nplanes)]
        else:
            starts = [int(v) for v in plane_offsets]
            if len(starts) != nplanes or any(v < 0 for v in starts):
                raise ValueError('SurfaceLayout: %s takes %d non-negative plane_offsets, got %r' % (format, nplanes, plane_offsets))
        first = y0 * pitch + x0 * bpp                                     # pixel (0, 0) in the first plane
        if kind == 'rgb':
            order = (2, 1, 0) if format.startswith('bgr') else (0, 1, 2)
            offset, pitches, step = [first + c for c in order], [pitch] * 3, [bpp] * 3
        elif nplanes == 0:                                               # yuyv / uyvy: x0 is even
            y_at, u_at, v_at = (0, 1, 3) if format == 'yuyv' else (1, 0, 2)
            offset, pitches, step = [first + y_at, first + u_at, first + v_at], [pitch] * 3, [2, 4, 4]
        elif nplanes == 1:                                               # nv12 / nv21 / p010: x0 and y0 are even
            at = starts[0] + (y0 // 2) * pitch + x0 * bpp                 # (x0 / 2 pairs of 2 * bpp bytes)
            u_at, v_at = (bpp, 0) if format == 'nv21' else (0, bpp)
            hi = bpp - 1                                                  # p010: the high byte of the little-endian word
            offset, pitches, step = [first + hi, at + u_at + hi, at + v_at + hi], [pitch] * 3, [bpp, 2 * bpp, 2 * bpp]
        else:                                                            # i420 / yv12
            at = [s_ + (y0 // 2) * cpitch + x0 // 2 for s_ in starts]
            u_at, v_at = (at[1], at[0]) if format == 'yv12' else (at[0], at[1])
            offset, pitches, step = [first, u_at, v_at], [pitch, cpitch, cpitch], [1, 1, 1]
        ends = [pitch * coded] + [s_ + cpitch * crows for s_ in starts]
        self.format, self.width, self.height, self.pitch, self.coded_height, self.x0, self.y0 = format, width, height, pitch, coded, x0, y0
        self.plane_offsets = tuple(starts)
        self.kind, self.xshift, self.yshift = kind, xs, ys
        self.offset, self.pitches, self.step = tuple(offset), tuple(pitches), tuple(step)
        self.frame_bytes = self.frame_stride = max(ends)
        for c in range(3):                                               # (plane_offsets can put a plane anywhere: the library's bound check)
            last = self.offset[c] + ((height - 1) >> (ys if c else 0)) * self.pitches[c] + ((width - 1) >> (xs if c else 0)) * self.step[c]
            if last >= self.frame_bytes:
                raise ValueError('SurfaceLayout: component %d reaches byte %d of a frame of %d bytes' % (c, last, self.frame_bytes))

    def descriptor(self):
        """-> the fields of eve_surface as a dict (struct_bytes left to the ctypes mirror)."""
        return dict(kind=0 if self.kind == 'rgb' else 1, width=self.width, height=self.height, frame_stride=self.frame_stride,
                    frame_bytes=self.frame_bytes, offset=self.offset, pitch=self.pitches, step=self.step, xshift=self.xshift,
                    yshift=self.yshift)

    def as_ctypes(self):
        """-> the _lib.Surface the entry points take."""
        import ctypes
        from ._lib import Surface
        d = self.descriptor()
        s = Surface()
        s.struct_bytes = ctypes.sizeof(Surface)
        for name in ('kind', 'width', 'height', 'frame_stride', 'frame_bytes', 'xshift', 'yshift'):
            setattr(s, name, d[name])
        for c in range(3):
            s.offset[c], s.pitch[c], s.step[c] = d['offset'][c], d['pitch'][c], d['step'][c]
        return s

    def key(self):
        return (self.format, self.width, self.height, self.pitch, self.coded_height, self.x0, self.y0, self.plane_offsets)

    def __eq__(self, other):
        return isinstance(other, SurfaceLayout) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'SurfaceLayout(%r, %d, %d, pitch=%d, coded_height=%d, x0=%d, y0=%d, plane_offsets=%r)' % self.key()


def surface_frames(frames, layout, lead, name='frames'):
    """A surface tensor checked against its layout -> (the frames as uint8 [N, frame_stride], the `lead` leading dimensions):
    contiguous uint8 whose trailing dimensions -- [rows, pitch], or flat -- multiply to layout.frame_stride.  lead=None: as many
    leading dimensions as leave such trailing ones (at least one).  TypeError for a wrong dtype, layout or number of dimensions,
    ValueError for a wrong size."""
    if not isinstance(layout, SurfaceLayout):
        raise TypeError('%s: the layout must be a data.SurfaceLayout, got %s' % (name, type(layout).__name__))
    if lead is None:
        lead, prod = 1, 1
        for i in range(getattr(frames, 'ndim', 0) - 1, 0, -1):
            prod *= int(frames.shape[i])
            if prod == layout.frame_stride:
                lead = i
                break
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() <= lead:
        raise TypeError('%s must be uint8 with %d leading dimension%s and one frame\'s bytes behind them, got %s %s' % (
            name, lead, '' if lead == 1 else 's', getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ()))))
    per_frame = 1
    for v in frames.shape[lead:]:
        per_frame *= int(v)
    if per_frame != layout.frame_stride:
        raise ValueError('%s: a frame holds %d bytes %s, the layout\'s frame_stride is %d (%r)' % (
            name, per_frame, tuple(frames.shape[lead:]), layout.frame_stride, layout))
    if not frames.is_contiguous():
        raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
    return frames.reshape(-1, per_frame), tuple(frames.shape[:lead])


def preprocess_frames(frames):
    flat, lead = _fold(frames)
    out = default_kernels().frames_u8_to_nchw(flat, EYE_SCALE, EYE_SHIFT)
    return out.view(lead + tuple(out.shape[1:]))


def preprocess_screen_frames(frames, size=None, bgr=False, format=None, matrix='bt601', layout=None):
    """size: None, or the (H, W) the network takes.  Frames of that size already (and size=None) are normalised as the
    reference normalises its 128 x 72 video; larger ones -- a live capture of the desktop, [..., IH, IW, 3 | 4] -- are
    area-averaged down to it by eve_screen_u8_area_to_nchw: the exact mean over each output pixel's footprint, fractional
    overlaps included, kept in float32.  A fourth channel (BGRA's alpha) is dropped there (so four-channel frames take that
    kernel at the target size too, where its values are the plain normalisation's bit for bit); the channel ORDER is kept as it
    comes unless bgr says otherwise.  The reference's own file was scaled by ffmpeg (bicubic, then
    lossy video coding): this is what a live stream can do instead, not a reproduction of it.
    bgr=True: the frames are BGR(A), as capture APIs and OpenCV deliver them; the planes come out in RGB order, bit for bit what
    the channel-reversed capture gives (eve_screen_u8_area_bgr_to_nchw, at every size: size=None takes the frames' own).
    format: None, or the layout a decoder or capture path delivers -- 'nv12' / 'i420' [..., IH*3/2, IW] (IH and IW even) or 'yuyv'
    [..., IH, IW, 2] (IW even), byte-linear per frame, with the integer matrix `matrix` ('bt601' or 'bt709', limited range, or
    'jfif', full range): every pixel is converted as it is read and the converted values are averaged, so the result equals the
    RGB call on the converted frame bit for bit and no RGB frame is made (eve_screen_area_fmt_to_nchw, at every size: size=None
    takes the frames' own).  bgr=True together with a format raises ValueError.
    layout: None, or a SurfaceLayout: the frames are then a decoder's or capture API's surface as it lies in memory, uint8
    [..., rows, pitch] or [..., frame_bytes] -- pitched rows, coded rows below the picture, a crop, NV21 / YV12 / UYVY / P010 or a
    pitched BGRA texture -- and the visible region is read through the layout's address rule inside the same launch
    (eve_screen_area_surface_to_nchw): the result equals the call on the de-pitched, cropped, byte-linear frame bit for bit and
    that copy is never made.  `matrix` applies to the YUV formats; bgr and format stay at their defaults (ValueError)."""
    if layout is not None:
        if bgr or format is not None:
            raise ValueError('preprocess_screen_frames: a layout names the format itself: leave bgr and format at their defaults')
        if not torch.is_tensor(frames) or frames.dim() < 2:
            raise TypeError('expected uint8 surface frames with at least one leading dimension, got %s' % (tuple(getattr(frames, 'shape', ())),))
        flat, lead = surface_frames(frames, layout, None)
        hw = (layout.height, layout.width) if size is None else (int(size[0]), int(size[1]))
        out = default_kernels().screen_area_surface_to_nchw(flat, hw, layout, matrix=matrix)
        return out.view(lead + tuple(out.shape[1:]))
    if format is not None:
        if bgr:
            raise ValueError('preprocess_screen_frames: bgr=True and format=%r exclude each other' % (format,))
        if format not in ('nv12', 'i420', 'yuyv'):
            raise ValueError("preprocess_screen_frames: format must be 'nv12', 'i420' or 'yuyv', got %r" % (format,))
        from .kernels import pixel_format_shape
        dims = 3 if format == 'yuyv' else 2                    # the planar layouts are [rows, IW]
        if not torch.is_tensor(frames) or frames.dim() < dims + 1:
            raise TypeError('expected uint8 %s frames with at least one leading dimension, got %s' % (format, tuple(getattr(frames, 'shape', ()))))
        lead = tuple(frames.shape[:-dims])
        flat = frames.reshape((-1,) + tuple(frames.shape[-dims:])).contiguous()
        IH, IW, _ = pixel_format_shape(flat, format, lead=1)
        hw = (IH, IW) if size is None else (int(size[0]), int(size[1]))
        out = default_kernels().screen_area_fmt_to_nchw(flat, hw, format, matrix=matrix)
        return out.view(lead + tuple(out.shape[1:]))
    flat, lead = _fold(frames)
    if bgr:
        hw = tuple(flat.shape[1:3]) if size is None else (int(size[0]), int(size[1]))
        out = default_kernels().screen_u8_area_bgr_to_nchw(flat, hw)
    elif size is None or (tuple(size) == tuple(flat.shape[1:3]) and flat.shape[3] == 3):
        out = default_kernels().frames_u8_to_nchw(flat, SCREEN_SCALE, None)
    else:
        out = default_kernels().screen_u8_area_to_nchw(flat, (int(size[0]), int(size[1])))
    return out.view(lead + tuple(out.shape[1:]))


def eye_patch_hw(config=None):
    """(H, W) of an eye patch: the config's eyes_size is (W, H), like screen_size."""
    if config is None:
        from .config import get_config
        config = get_config()
    return int(config.eyes_size[1]), int(config.eyes_size[0])


def camera_lens(camera_matrix, dist_coeffs):
    """The lens rows of a calibrated camera: camera_matrix [..., 3, 3] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] and dist_coeffs
    [..., n] with OpenCV's n = 4, 5 or 8 coefficients in OpenCV's order k1, k2, p1, p2[, k3[, k4, k5, k6]] (cv2.calibrateCamera's
    result, flattened) -> float32 [..., 12] = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6), the missing coefficients zero.
    numpy arrays or torch tensors; the leading dimensions broadcast against each other (one distortion vector for a batch of
    matrices, say).  A torch tensor comes back when camera_matrix is one (on its device), else a numpy array.

    ValueError: 12 or 14 coefficients (thin-prism and tilt terms are not offered), any other count, a non-zero skew K[0, 1], a last
    row other than (0, 0, 1).  All-zero coefficients are fine: such a row takes the plain warp, bit for bit."""
    as_torch = torch.is_tensor(camera_matrix)
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    K, d = to_np(camera_matrix).astype(np.float64), to_np(dist_coeffs).astype(np.float64)
    if K.ndim < 2 or K.shape[-2:] != (3, 3):
        raise ValueError('camera_lens: camera_matrix must be [..., 3, 3], got %s' % (tuple(K.shape),))
    if d.ndim < 1 or d.shape[-1] not in (4, 5, 8):
        raise ValueError('camera_lens: 4, 5 or 8 distortion coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got %s%s' % (
            tuple(d.shape), ': thin-prism and tilt coefficients are not offered' if d.ndim and d.shape[-1] in (12, 14) else ''))
    if (K[..., 0, 1] != 0).any():
        raise ValueError('camera_lens: a skewed camera matrix (K[0, 1] != 0) is not offered')
    if (K[..., 2, :] != np.array([0.0, 0.0, 1.0])).any():
        raise ValueError('camera_lens: the last row of camera_matrix must be (0, 0, 1)')
    lead = np.broadcast_shapes(K.shape[:-2], d.shape[:-1])
    out = np.zeros(lead + (12,), dtype=np.float32)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]
    out[..., 4:4 + d.shape[-1]] = d
    return torch.from_numpy(out).to(camera_matrix.device) if as_torch else out


def eye_pose(camera_matrix, head_rvec, head_tvec, eye_centers, focal_norm, distance_norm):
    """The pose rows of the `eye_pose` key, from what a face tracker holds per frame: camera_matrix [..., 3, 3] =
    [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] of the UNDISTORTED image (with camera_lens, normally the same K); head_rvec [..., 3] or
    [..., 3, 1] and head_tvec likewise, cv2.solvePnP's result for the head model; eye_centers [..., 2, 3], the left and the right
    eye's centre in the head model's coordinates and in head_tvec's length unit (EVE: millimetres); focal_norm and distance_norm
    (scalars or [...]): the virtual camera the patches are normalised to -- focal length in patch pixels and distance in that
    length unit.  Both are required: the reference does not state the values behind its own patches, and no default here
    pretends to.  -> float32 [..., 18] = (fx, fy, cx, cy, r0, r1, r2, t0, t1, t2, l0, l1, l2, q0, q1, q2, focal_norm,
    distance_norm).  numpy arrays or torch tensors; the leading dimensions broadcast against each other (one camera matrix
    and one head model for a clip, say).  A torch tensor comes back when camera_matrix is one (on its device), else a numpy array.

    ValueError: a camera matrix that is not [..., 3, 3], has skew (K[0, 1] != 0) or a last row other than (0, 0, 1); vectors or
    eye centres of another shape.  Values are not judged here: a NaN or a head behind the camera gives pose_valid False on the
    device (include/eve_hip.h eve_eye_pose_normalize)."""
    as_torch = torch.is_tensor(camera_matrix)
    to_np = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)
    K, r, t, c = to_np(camera_matrix), to_np(head_rvec), to_np(head_tvec), to_np(eye_centers)
    f, dn = to_np(focal_norm), to_np(distance_norm)
    if K.ndim < 2 or K.shape[-2:] != (3, 3):
        raise ValueError('eye_pose: camera_matrix must be [..., 3, 3], got %s' % (tuple(K.shape),))
    if (K[..., 0, 1] != 0).any():
        raise ValueError('eye_pose: a skewed camera matrix (K[0, 1] != 0) is not offered')
    if (K[..., 2, :] != np.array([0.0, 0.0, 1.0])).any():
        raise ValueError('eye_pose: the last row of camera_matrix must be (0, 0, 1)')
    vecs = []
    for name, v in (('head_rvec', r), ('head_tvec', t)):
        if v.ndim >= 2 and v.shape[-2:] == (3, 1):
            v = v[..., 0]
        if v.ndim < 1 or v.shape[-1] != 3:
            raise ValueError('eye_pose: %s must be [..., 3] or [..., 3, 1], got %s' % (name, tuple(v.shape)))
        vecs.append(v)
    if c.ndim < 2 or c.shape[-2:] != (2, 3):
        raise ValueError('eye_pose: eye_centers must be [..., 2, 3] (left, right), got %s' % (tuple(c.shape),))
    lead = np.broadcast_shapes(K.shape[:-2], vecs[0].shape[:-1], vecs[1].shape[:-1], c.shape[:-2], f.shape, dn.shape)
    out = np.zeros(lead + (18,), dtype=np.float32)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]
    out[..., 4:7], out[..., 7:10] = vecs
    out[..., 10:13], out[..., 13:16] = c[..., 0, :], c[..., 1, :]
    out[..., 16], out[..., 17] = f, dn
    return torch.from_numpy(out).to(camera_matrix.device) if as_torch else out


def normalize_eyes(pose, size=None):
    """Eye normalisation from pose rows, on the device: pose float32 [..., 18] (eye_pose) -> a dict of head_R [..., 3, 3],
    left_o / right_o [..., 3], left_R / right_R [..., 3, 3], left_eye_warp / right_eye_warp [..., 3, 3], left_h / right_h [..., 2]
    (float32) and pose_valid, bool [..., 2] (left, right): what a batch with `camera_frame` + `eye_pose` is given before the
    networks run.  size: (H, W) of the eye patch, default the config's eyes_size.

    The formulas are the published normalisation procedure the reference cites for the values it ships precomputed (Zhang et al.
    2018, "Revisiting data normalization for appearance-based gaze estimation"): <side>_R has the rows (right, down, forward)
    with forward the direction of the eye's origin o = head_R c + t and right orthogonal to the head's x axis; <side>_eye_warp is
    inv(W) of W = Kn S R K^-1, S = diag(1, 1, distance_norm / |o|), in closed form and not rescaled; <side>_h = (asin M12,
    atan2(M02, M22)) of M = R head_R, so head_R = Rx(a) seen on the optical axis gives h = (-a, 0) and Ry(b) gives (0, b).  None of
    it could be compared with the EVE dataset's own values: the dataset is on no machine this package was built on.  An eye with
    pose_valid False (a NaN, a non-positive focal length or distance, an origin behind the camera, a head x axis along the line
    of sight) has a zero warp -- a black patch -- R = I, o = 0, h = 0.  The contract is include/eve_hip.h eve_eye_pose_normalize."""
    if not torch.is_tensor(pose) or pose.dtype != torch.float32 or pose.dim() < 1 or pose.shape[-1] != 18:
        raise TypeError('expected float32 pose rows shaped [..., 18], got %s %s' % (getattr(pose, 'dtype', type(pose)),
                                                                                   tuple(getattr(pose, 'shape', ()))))
    if pose.numel() == 0:
        raise ValueError('normalize_eyes: no pose rows (shape %s)' % (tuple(pose.shape),))
    lead = tuple(pose.shape[:-1])
    hw = eye_patch_hw() if size is None else (int(size[0]), int(size[1]))
    head_R, o, R, warp, h, valid = default_kernels().eye_pose_normalize(pose.reshape(-1, 18).contiguous(), hw)
    out = {'head_R': head_R.view(lead + (3, 3))}
    for e, side in enumerate(('left', 'right')):
        out[side + '_o'] = o[e].view(lead + (3,))
        out[side + '_R'] = R[e].view(lead + (3, 3))
        out[side + '_eye_warp'] = warp[e].view(lead + (3, 3))
        out[side + '_h'] = h[e].view(lead + (2,))
    out['pose_valid'] = valid.view((2,) + lead).movedim(0, -1) != 0
    return out


def face_rig(camera_matrix, face_model, eye_centers, focal_norm, distance_norm):
    """The rows of the `face_rig` key, one per sequence: camera_matrix [..., 3, 3] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] of the
    UNDISTORTED image the landmarks refer to; face_model [..., L, 3], the head model's points in the order the tracker delivers
    its landmarks, 4 <= L <= 68; eye_centers [..., 2, 3], left and right, in the same frame and length unit (EVE: millimetres);
    focal_norm and distance_norm (scalars or [...]) as for eye_pose.  -> float32 [..., 12 + 3L] = (fx, fy, cx, cy, left eye
    centre, right eye centre, focal_norm, distance_norm, the L model points).  numpy arrays or torch tensors; the leading
    dimensions broadcast against each other.  A torch tensor comes back when camera_matrix is one (on its device), else a numpy
    array.

    ValueError: a camera matrix that is not [..., 3, 3], has skew (K[0, 1] != 0) or a last row other than (0, 0, 1); a model
    that is not [..., L, 3] with L in 4..68; eye centres of another shape.  Values are not judged here: a NaN, or model points
    on one line, give valid False on the device (include/eve_hip.h eve_face_pose_solve)."""
    as_torch = torch.is_tensor(camera_matrix)
    to_np = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)
    K, m, c, f, dn = to_np(camera_matrix), to_np(face_model), to_np(eye_centers), to_np(focal_norm), to_np(distance_norm)
    if K.ndim < 2 or K.shape[-2:] != (3, 3):
        raise ValueError('face_rig: camera_matrix must be [..., 3, 3], got %s' % (tuple(K.shape),))
    if (K[..., 0, 1] != 0).any():
        raise ValueError('face_rig: a skewed camera matrix (K[0, 1] != 0) is not offered')
    if (K[..., 2, :] != np.array([0.0, 0.0, 1.0])).any():
        raise ValueError('face_rig: the last row of camera_matrix must be (0, 0, 1)')
    if m.ndim < 2 or m.shape[-1] != 3 or not 4 <= m.shape[-2] <= 68:
        raise ValueError('face_rig: face_model must be [..., L, 3] with 4 <= L <= 68, got %s' % (tuple(m.shape),))
    if c.ndim < 2 or c.shape[-2:] != (2, 3):
        raise ValueError('face_rig: eye_centers must be [..., 2, 3] (left, right), got %s' % (tuple(c.shape),))
    L = m.shape[-2]
    lead = np.broadcast_shapes(K.shape[:-2], m.shape[:-2], c.shape[:-2], f.shape, dn.shape)
    out = np.zeros(lead + (12 + 3 * L,), dtype=np.float32)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]
    out[..., 4:7], out[..., 7:10] = c[..., 0, :], c[..., 1, :]
    out[..., 10], out[..., 11] = f, dn
    out[..., 12:] = m.reshape(m.shape[:-2] + (3 * L,))
    return torch.from_numpy(out).to(camera_matrix.device) if as_torch else out


def check_huber_px(huber_px, where):
    """None or a finite number > 0 (pixels) -> None or float; anything else raises ValueError."""
    if huber_px is None:
        return None
    if isinstance(huber_px, bool) or not isinstance(huber_px, (int, float)) or not 0 < huber_px < float('inf'):
        raise ValueError('%s: huber_px must be None or a finite number > 0 (pixels), got %r' % (where, huber_px))
    return float(huber_px)


def undistort_points(points, lens):
    """Raw-frame pixels -> pixels of the undistorted image, on the device, in place of cv2.undistortPoints(..., P=K) on the host:
    points float32 [..., 2] = (u, v); lens float32 [..., 12] rows from camera_lens with the same leading dimensions, or one row
    [12] for all points.  -> (float64 [..., 2] = (fx*x + cx, fy*y + cy) with the row's own intrinsics, ok bool [...]).  Newton's
    method on the forward model of the eye-warp kernels (include/eve_hip.h eve_undistort_points): exact to a few 1e-16 in
    normalised coordinates after at most 5 steps on ordinary lenses, where OpenCV's five fixed-point passes leave up to 1e-4.
    ok False (and a zero point): the iteration gave up (12 steps), the point lies at or beyond a pole of the rational model, a
    NaN.  Beyond the fold-back radius of a strong barrel polynomial the model is not invertible and which pre-image is found is
    not promised."""
    ok = lambda t: torch.is_tensor(t) and t.dtype == torch.float32
    if not ok(points) or points.dim() < 1 or points.shape[-1] != 2 or points.numel() == 0:
        raise TypeError('expected float32 points shaped [..., 2], got %s %s' % (getattr(points, 'dtype', type(points)),
                                                                                tuple(getattr(points, 'shape', ()))))
    lead = tuple(points.shape[:-1])
    if not ok(lens) or (tuple(lens.shape) != (12,) and tuple(lens.shape) != lead + (12,)):
        raise TypeError('expected float32 lens rows shaped %s or (12,), got %s %s' % (lead + (12,), getattr(lens, 'dtype', type(lens)),
                                                                                    tuple(getattr(lens, 'shape', ()))))
    rows = lens.reshape(-1, 12).contiguous()
    xy, good = default_kernels().undistort_points(points.reshape(-1, 2).contiguous(), rows)
    rows = rows.to(torch.float64)
    px = torch.stack([rows[:, 0] * xy[:, 0] + rows[:, 2], rows[:, 1] * xy[:, 1] + rows[:, 3]], dim=-1)
    good = good != 0
    return torch.where(good[:, None], px, torch.zeros_like(px)).view(lead + (2,)), good.view(lead)


def solve_head_pose(landmarks, rig, lengths=None, lens=None, huber_px=None):
    """The head pose of every frame from its 2-D face landmarks, on the device, in place of one cv2.solvePnP per frame: landmarks
    float32 [S, T, L, 2 | 3] (or [T, L, 2 | 3] with rig [12 + 3L]: one sequence) = pixel (u, v[, w]) of the undistorted image, w an
    optional confidence (0 drops the point); rig float32 [S, 12 + 3L] from face_rig, one row per sequence; lengths None, or S
    integers (a list, a numpy array or a tensor): frames past a sequence's count are not solved.  -> a dict of head_R [S, T, 3, 3],
    head_t [S, T, 3], reproj_rms [S, T] (pixels) float32 and valid, bool [S, T].  Every sequence starts cold (a closed-form guess),
    every later frame from the frame before; a frame without a solution (a NaN, fewer than 4 weighted points, model points on a
    line, no convergence) has valid False, head_R = I, head_t = 0, reproj_rms = 0, and the next one starts cold.  Levenberg-
    Marquardt on the weighted reprojection error in float64; the contract is include/eve_hip.h eve_face_pose_solve.  Not
    offered: RANSAC, an rvec, gradients, per-frame camera matrices; a planar model runs, but which of its two minima is found is
    not promised.

    lens: None, or float32 [S, T, 12] rows from camera_lens ([T, 12] for one sequence) -- the landmarks are then pixels of the RAW
    frame, as a tracker fed the raw frame reports them: each is undistorted on the device (undistort_points' iteration; a point
    it cannot invert is dropped like one of weight 0) and the rig keeps describing the undistorted image.  huber_px: None, or
    k > 0 in pixels -- a Huber loss: a landmark further than k from its reprojection pulls with k / distance of its weight, so a
    few landmarks that are confidently wrong (a hand, hair) no longer tilt the head; k = 3 suits 1 px of landmark noise.  A
    frame that ends with fewer than 4 landmarks within k is invalid.  With either argument the result gains inliers, uint8
    [S, T]: the landmarks within k, or the used ones without the loss, 0 where invalid (include/eve_hip.h
    eve_face_pose_solve_ex); reproj_rms stays the weighted rms over ALL used landmarks.  Not promised: very few landmarks (L = 6)
    with an outlier among them.  Without both, exactly what this function always returned."""
    ok = lambda t: torch.is_tensor(t) and t.dtype == torch.float32
    if not ok(landmarks) or landmarks.dim() not in (3, 4) or landmarks.shape[-1] not in (2, 3):
        raise TypeError('expected float32 landmarks shaped [S, T, L, 2 | 3], got %s %s' % (getattr(landmarks, 'dtype', type(landmarks)),
                                                                                          tuple(getattr(landmarks, 'shape', ()))))
    single = landmarks.dim() == 3
    if single:
        landmarks = landmarks[None]
        rig = rig[None] if ok(rig) and rig.dim() == 1 else rig
    S, T, L = landmarks.shape[:3]
    if not ok(rig) or tuple(rig.shape) != (S, 12 + 3 * L):
        raise TypeError('expected float32 rig rows shaped %s, got %s %s' % ((S, 12 + 3 * L), getattr(rig, 'dtype', type(rig)),
                                                                           tuple(getattr(rig, 'shape', ()))))
    if landmarks.numel() == 0:
        raise ValueError('solve_head_pose: no frames (shape %s)' % (tuple(landmarks.shape),))
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=landmarks.device, dtype=torch.int32).contiguous()
        if tuple(lengths.shape) != (S,):
            raise ValueError('solve_head_pose: lengths needs one entry per sequence (%d)' % S)
    if lens is None and huber_px is None:
        head_R, head_t, rms, valid = default_kernels().face_pose_solve(landmarks.contiguous(), rig.contiguous(), lengths)
        out = {'head_R': head_R, 'head_t': head_t, 'reproj_rms': rms, 'valid': valid != 0}
        return {k_: v[0] for k_, v in out.items()} if single else out
    if lens is not None:
        lens = lens[None] if single and ok(lens) and lens.dim() == 2 else lens
        if not ok(lens) or tuple(lens.shape) != (S, T, 12):
            raise TypeError('expected float32 lens rows shaped %s, got %s %s' % ((S, T, 12), getattr(lens, 'dtype', type(lens)),
                                                                                tuple(getattr(lens, 'shape', ()))))
        lens = lens.contiguous()
    head_R, head_t, rms, valid, inliers = default_kernels().face_pose_solve_ex(landmarks.contiguous(), rig.contiguous(), lens,
                                                                               check_huber_px(huber_px, 'solve_head_pose'), lengths)
    out = {'head_R': head_R, 'head_t': head_t, 'reproj_rms': rms, 'valid': valid != 0, 'inliers': inliers}
    return {k_: v[0] for k_, v in out.items()} if single else out


def check_huber_mm(huber_mm, where):
    """None or a finite number > 0 (millimetres on the screen) -> None or float; anything else raises ValueError."""
    if huber_mm is None:
        return None
    if isinstance(huber_mm, bool) or not isinstance(huber_mm, (int, float)) or not 0 < huber_mm < float('inf'):
        raise ValueError('%s: huber_mm must be None or a finite number > 0 (millimetres), got %r' % (where, huber_mm))
    return float(huber_mm)


def check_min_samples(min_samples, where):
    if isinstance(min_samples, bool) or not isinstance(min_samples, int) or min_samples < 1:
        raise ValueError('%s: min_samples must be an integer >= 1, got %r' % (where, min_samples))
    return min_samples


def calibration_samples(g, head_R, origin, R, inv_camera_transformation, pixels_per_millimeter, target_px):
    """What the per-person offset fit needs of N frames of ONE eye, reduced on the device: g float32 [N, 2] (the network's
    <side>_g_initial), head_R [N, 3, 3], origin [N, 3] (<side>_o), R [N, 3, 3] (<side>_R), inv_camera_transformation [N, 4, 4],
    pixels_per_millimeter [N, 2] and target_px [N, 2], the dot the person looked at in actual_screen_size pixels.  -> float64
    [N, 16], row i for frame i: A (9), e (3), the target in millimetres (2), the weight 1.0, 0.0 (include/eve_hip.h
    eve_calib_append).  A frame that is not usable -- a value that is not finite, a target behind the eye -- gives a row of zeros,
    which fit_gaze_offset passes over (its weight is 0)."""
    ok = lambda t: torch.is_tensor(t) and t.dtype == torch.float32
    if not ok(g) or g.dim() != 2 or g.shape[1] != 2 or g.shape[0] < 1:
        raise TypeError('calibration_samples: g must be float32 [N, 2] with N >= 1, got %s %s' % (getattr(g, 'dtype', type(g)),
                                                                                                 tuple(getattr(g, 'shape', ()))))
    N = g.shape[0]
    for name, t, shape in (('head_R', head_R, (N, 3, 3)), ('origin', origin, (N, 3)), ('R', R, (N, 3, 3)),
                           ('inv_camera_transformation', inv_camera_transformation, (N, 4, 4)),
                           ('pixels_per_millimeter', pixels_per_millimeter, (N, 2)), ('target_px', target_px, (N, 2))):
        if not ok(t) or tuple(t.shape) != shape:
            raise TypeError('calibration_samples: %s must be float32 %s, got %s %s' % (name, list(shape), getattr(t, 'dtype', type(t)),
                                                                                      tuple(getattr(t, 'shape', ()))))
    dev = g.device
    samples = torch.zeros((N, 1, 1, 16), dtype=torch.float64, device=dev)
    count, dropped = torch.zeros((N, 1), dtype=torch.int32, device=dev), torch.zeros((N, 1), dtype=torch.int32, device=dev)
    c = lambda t, *s: t.reshape((N, 1) + s).contiguous()
    default_kernels().calib_append(c(g, 2)[None], c(head_R, 3, 3), c(origin, 3)[None], c(R, 3, 3)[None], c(inv_camera_transformation, 4, 4),
                                   c(pixels_per_millimeter, 2), c(target_px, 2), samples, count, dropped)
    return samples.view(N, 16)


def fit_gaze_offset(samples, counts=None, huber_mm=None, min_samples=5):
    """The per-person offset kappa = (pitch, yaw) between the optical axis EyeNet sees and the visual axis, fitted on the device to
    calibration samples: samples float64 [S, C, 16] ([C, 16]: one sequence) as calibration_samples or an EVEStream's store holds
    them; counts None (all C rows) or S integers (a list, a numpy array or a tensor): the rows in use.  Levenberg-Marquardt from
    kappa = 0 on sum rho(|PoG_i(kappa) - target_i|) in millimetres, rho the square, or with huber_mm a Huber loss whose threshold
    is that many millimetres on the screen (25 suits 8 mm of fixation noise).  -> a dict of kappa float64 [S, 2] (radians), rms_mm
    float64 [S] (over all used samples), used and inliers int32 [S] (the samples within huber_mm; used without the loss) and ok
    bool [S].  ok False (kappa, rms_mm, inliers 0): fewer than min_samples rows with weight > 0, a system that is not positive
    definite (every target on one line through the eye, say), no convergence, or |kappa| above 0.35 rad (20 degrees: the fit
    diverged).  One launch, a wavefront per sequence; the host does not wait.  The contract, summation order included, is
    include/eve_hip.h eve_calib_fit and tests/calib_ref.py.  Not offered: per-sample weights (entry 14 of a row is 1.0, or 0.0 for
    an absent row), gradients; the residual that depends on the position on the screen is fit_screen_map's."""
    if not torch.is_tensor(samples) or samples.dtype != torch.float64 or samples.dim() not in (2, 3) or samples.shape[-1] != 16:
        raise TypeError('fit_gaze_offset: samples must be float64 [S, C, 16], got %s %s' % (getattr(samples, 'dtype', type(samples)),
                                                                                          tuple(getattr(samples, 'shape', ()))))
    single = samples.dim() == 2
    if single:
        samples = samples[None]
    if samples.numel() == 0:
        raise ValueError('fit_gaze_offset: no samples (shape %s)' % (tuple(samples.shape),))
    S = samples.shape[0]
    huber_mm, min_samples = check_huber_mm(huber_mm, 'fit_gaze_offset'), check_min_samples(min_samples, 'fit_gaze_offset')
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=samples.device, dtype=torch.int32).contiguous()
        if tuple(counts.shape) != (S,):
            raise ValueError('fit_gaze_offset: counts needs one entry per sequence (%d)' % S)
    kappa, rms, used, inliers, good = default_kernels().calib_fit(samples.contiguous(), counts, None, huber_mm, min_samples)
    out = {'kappa': kappa, 'rms_mm': rms, 'used': used, 'inliers': inliers, 'ok': good != 0}
    return {k_: v[0] for k_, v in out.items()} if single else out


# ---------------------------------------------------------------------------------------------------------------- the screen-space map
SCREEN_MODELS = {'offset': 1, 'affine': 2, 'quadratic': 3}      # the kind byte (0: no map) -> 1, 3, 6 terms of (1, u, v, u*u, u*v, v*v)
SCREEN_CALIB_REPORT = ('rms_mm', 'mean_mm', 'max_mm', 'mean_deg', 'rms_mm_raw', 'mean_mm_raw', 'max_mm_raw', 'mean_deg_raw')


def check_screen_model(model, where):
    """'offset', 'affine' or 'quadratic' -> the kind byte 1, 2, 3; anything else raises ValueError."""
    if not isinstance(model, str) or model not in SCREEN_MODELS:
        raise ValueError("%s: model must be 'offset', 'affine' or 'quadratic', got %r" % (where, model))
    return SCREEN_MODELS[model]


def check_max_shift_mm(max_shift_mm, where):
    """A finite number > 0 (millimetres on the screen) -> float; anything else raises ValueError."""
    if isinstance(max_shift_mm, bool) or not isinstance(max_shift_mm, (int, float)) or not 0 < max_shift_mm < float('inf'):
        raise ValueError('%s: max_shift_mm must be a finite number > 0 (millimetres), got %r' % (where, max_shift_mm))
    return float(max_shift_mm)


def check_screen_min_samples(min_samples, where):
    """None (the model's number of terms decides) or an integer >= 1 -> int."""
    return 1 if min_samples is None else check_min_samples(min_samples, where)


def check_screen_size(screen_size, where):
    """(W, H), two finite numbers > 0 -> (float, float); anything else raises ValueError."""
    try:
        W, H = screen_size
        ok = all(not isinstance(v, bool) and isinstance(v, (int, float)) and 0 < v < float('inf') for v in (W, H))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%s: screen_size must be (W, H), two finite numbers > 0 (actual_screen_size), got %r' % (where, screen_size))
    return float(W), float(H)


def screen_calibration_samples(pog_px, o, inv_camera_transformation, pixels_per_millimeter, target_px, screen_size):
    """What the screen-space map's fit needs of N frames, reduced on the device: pog_px float32 [N, 2] (the pipeline's output point,
    PoG_px_final or PoG_px_initial, uncorrected), o [N, 3] (the binocular origin), inv_camera_transformation [N, 4, 4],
    pixels_per_millimeter [N, 2], target_px [N, 2] (the dot the person looked at) and screen_size = actual_screen_size (W, H).
    -> float64 [N, 12], row i for frame i: u, v, the point and the target in millimetres (2 + 2), the eye in screen coordinates
    (3), the weight 1.0, two reserved 0.0 (include/eve_hip.h eve_screen_calib_append).  A frame that is not usable -- a value that
    is not finite, a pixels_per_millimeter that is not > 0, an eye in the screen plane -- gives a row of zeros, which fit_screen_map
    passes over (its weight is 0)."""
    ok = lambda t: torch.is_tensor(t) and t.dtype == torch.float32
    if not ok(pog_px) or pog_px.dim() != 2 or pog_px.shape[1] != 2 or pog_px.shape[0] < 1:
        raise TypeError('screen_calibration_samples: pog_px must be float32 [N, 2] with N >= 1, got %s %s' % (
            getattr(pog_px, 'dtype', type(pog_px)), tuple(getattr(pog_px, 'shape', ()))))
    N = pog_px.shape[0]
    for name, t, shape in (('o', o, (N, 3)), ('inv_camera_transformation', inv_camera_transformation, (N, 4, 4)),
                           ('pixels_per_millimeter', pixels_per_millimeter, (N, 2)), ('target_px', target_px, (N, 2))):
        if not ok(t) or tuple(t.shape) != shape:
            raise TypeError('screen_calibration_samples: %s must be float32 %s, got %s %s' % (name, list(shape), getattr(t, 'dtype', type(t)),
                                                                                             tuple(getattr(t, 'shape', ()))))
    size = check_screen_size(screen_size, 'screen_calibration_samples')
    dev = pog_px.device
    samples = torch.zeros((N, 1, 12), dtype=torch.float64, device=dev)
    count, dropped = torch.zeros((N,), dtype=torch.int32, device=dev), torch.zeros((N,), dtype=torch.int32, device=dev)
    c = lambda t, *s: t.reshape((N, 1) + s).contiguous()
    default_kernels().screen_calib_append(c(pog_px, 2), c(o, 3), c(inv_camera_transformation, 4, 4), c(pixels_per_millimeter, 2),
                                          c(target_px, 2), size, samples, count, dropped)
    return samples.view(N, 12)


def _screen_samples_arg(samples, counts, where):
    if not torch.is_tensor(samples) or samples.dtype != torch.float64 or samples.dim() not in (2, 3) or samples.shape[-1] != 12:
        raise TypeError('%s: samples must be float64 [S, C, 12], got %s %s' % (where, getattr(samples, 'dtype', type(samples)),
                                                                              tuple(getattr(samples, 'shape', ()))))
    single = samples.dim() == 2
    if single:
        samples = samples[None]
    if samples.numel() == 0:
        raise ValueError('%s: no samples (shape %s)' % (where, tuple(samples.shape)))
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=samples.device, dtype=torch.int32).contiguous()
        if tuple(counts.shape) != (samples.shape[0],):
            raise ValueError('%s: counts needs one entry per stream (%d)' % (where, samples.shape[0]))
    return samples.contiguous(), counts, single


def _screen_fit_result(res, kind, single):
    coef, report, used, inliers, solves, good = res
    out = {'coef': coef, 'kind': kind, 'ok': good != 0, 'used': used, 'inliers': inliers, 'solves': solves}
    out.update({name: report[:, i] for i, name in enumerate(SCREEN_CALIB_REPORT)})
    return {k_: v[0] for k_, v in out.items()} if single else out


def fit_screen_map(samples, counts=None, model='affine', huber_mm=None, min_samples=None, max_shift_mm=100.0):
    """The screen-space map fitted on the device to calibration samples: samples float64 [S, C, 12] ([C, 12]: one stream) as
    screen_calibration_samples or an EVEStream's store holds them; counts None (all C rows) or S integers: the rows in use.  model:
    'offset', 'affine' (default) or 'quadratic'; huber_mm None (least squares) or a Huber threshold in millimetres (25 suits 8 mm of
    fixation noise); min_samples None (the model's number of terms) or more; max_shift_mm: the longest correction at a sample the
    fit may produce.  -> a dict of coef float64 [S, 2, 6] (axis, term; millimetres), kind uint8 [S] (the model's byte where ok, else
    0), ok bool [S], used, inliers, solves int32 [S] and the report float64 [S]: rms_mm, mean_mm, max_mm, mean_deg of the corrected
    point and the same with _raw of the uncorrected one.  ok False (everything but used 0): too few rows with weight > 0, dots that
    do not determine the model, no convergence within 64 solves, a correction above max_shift_mm.  One launch, a wavefront per
    stream; the host does not wait.  The contract, summation order included, is include/eve_hip.h eve_screen_calib_fit and
    tests/screen_calib_ref.py.  Not offered: per-sample weights from the caller (entry 9 of a row is 1.0, or 0.0 for an absent
    row), cubic or higher models, automatic recalibration, gradients."""
    samples, counts, single = _screen_samples_arg(samples, counts, 'fit_screen_map')
    kind = check_screen_model(model, 'fit_screen_map')
    huber_mm, max_shift_mm = check_huber_mm(huber_mm, 'fit_screen_map'), check_max_shift_mm(max_shift_mm, 'fit_screen_map')
    min_samples = check_screen_min_samples(min_samples, 'fit_screen_map')
    res = default_kernels().screen_calib_fit(samples, counts, None, 0, kind, huber_mm, min_samples, max_shift_mm)
    return _screen_fit_result(res, (res[5] != 0).to(torch.uint8) * kind, single)


def _screen_map_arg(coef, kind, S, device, where):
    coef = torch.as_tensor(coef, dtype=torch.float64).to(device)
    kind = torch.as_tensor(kind)
    if coef.dim() == 2 and kind.dim() == 0:
        coef, kind = coef[None].expand(S, 2, 6), kind[None].expand(S)
    if tuple(coef.shape) != (S, 2, 6):
        raise ValueError('%s: coef must be [%d, 2, 6] (stream, axis, term), got %s' % (where, S, tuple(coef.shape)))
    if tuple(kind.shape) != (S,) or kind.dtype.is_floating_point or kind.dtype == torch.bool:
        raise ValueError('%s: kind must be %d integers in 0 .. 3 (none, offset, affine, quadratic)' % (where, S))
    return coef.contiguous(), kind.to(device=device, dtype=torch.uint8).contiguous()


def evaluate_screen_map(samples, coef, kind, counts=None):
    """The accuracy of given maps over samples -- the validation pass -- on the device: samples and counts as fit_screen_map takes
    them, coef [S, 2, 6] and kind S integers in 0 .. 3 (or one [2, 6] map and one kind for every stream).  -> fit_screen_map's dict
    with solves 0, inliers = used and ok where a row is present; a map of kind 0 reports the raw numbers in both sets.  Nothing is
    solved (eve_screen_calib_fit in mode 1)."""
    samples, counts, single = _screen_samples_arg(samples, counts, 'evaluate_screen_map')
    coef, kind = _screen_map_arg(coef, kind, samples.shape[0], samples.device, 'evaluate_screen_map')
    res = default_kernels().screen_calib_fit(samples, counts, None, 1, 0, None, 1, 100.0, coef, kind)
    return _screen_fit_result(res, kind, single)


def apply_screen_map(pog_px, pixels_per_millimeter, coef, kind, screen_size):
    """The screen-space map applied on the device: pog_px float32 [B, T, 2] ([T, 2]: one stream), pixels_per_millimeter the same
    shape, coef [B, 2, 6] and kind B integers in 0 .. 3 (one [2, 6] map and one kind for one stream), screen_size (W, H) -> the
    corrected point, float32 of pog_px's shape, clamped to the screen; a stream of kind 0 gets its input bits
    (include/eve_hip.h eve_screen_calib_apply)."""
    ok = lambda t: torch.is_tensor(t) and t.dtype == torch.float32
    if not ok(pog_px) or pog_px.dim() not in (2, 3) or pog_px.shape[-1] != 2 or pog_px.numel() == 0:
        raise TypeError('apply_screen_map: pog_px must be float32 [B, T, 2], got %s %s' % (getattr(pog_px, 'dtype', type(pog_px)),
                                                                                         tuple(getattr(pog_px, 'shape', ()))))
    if not ok(pixels_per_millimeter) or tuple(pixels_per_millimeter.shape) != tuple(pog_px.shape):
        raise TypeError('apply_screen_map: pixels_per_millimeter must be float32 %s, got %s %s' % (
            list(pog_px.shape), getattr(pixels_per_millimeter, 'dtype', type(pixels_per_millimeter)),
            tuple(getattr(pixels_per_millimeter, 'shape', ()))))
    size = check_screen_size(screen_size, 'apply_screen_map')
    single = pog_px.dim() == 2
    px, ppm = (pog_px[None], pixels_per_millimeter[None]) if single else (pog_px, pixels_per_millimeter)
    coef, kind = _screen_map_arg(coef, kind, px.shape[0], px.device, 'apply_screen_map')
    out = default_kernels().screen_calib_apply(px.contiguous(), ppm.contiguous(), coef, kind, size)
    return out[0] if single else out


def warp_eye_patches(frames, warps, size=None, lens=None, format='rgb', matrix='bt601', layout=None):
    """One eye's patches cut from whole camera frames on the device, in place of two cv2.warpPerspective calls per frame on the
    host: frames uint8 [..., IH, IW, 3 | 4] (a fourth channel ignored, the channel order kept), warps float32 [..., 3, 3] with the
    same leading dimensions -> float32 [..., 3, H, W] in [-1, 1], the values preprocess_frames gives for the cut patch.  size:
    (H, W), default the config's eyes_size.

    warps[i] maps a PATCH pixel (x, y, 1) to a CAMERA pixel (X / Wd, Y / Wd) -- the matrix cv2.warpPerspective uses with
    WARP_INVERSE_MAP.  The EVE pipeline's perspective-normalisation matrix W maps the camera to the patch
    (cv2.warpPerspective(frame, W, (w, h))): pass inv(W).  Sampling is bilinear with 8 fractional bits per axis and zero outside
    the frame (which comes out as -1.0), bit-exact by the contract of include/eve_hip.h eve_eye_warp_u8_to_nchw.

    lens: None for frames that are already undistorted (what the EVE dataset's videos are), or float32 [..., 12] rows from
    camera_lens with the same leading dimensions for RAW frames: W and inv(W) then refer to the undistorted image as before, and
    every coordinate goes through the camera's distortion model before the frame is read (eve_eye_warp_lens_u8_to_nchw).  No
    undistorted frame is made.  A row with zero coefficients gives the lens=None bits.

    format: 'rgb' (above), or the layout a camera or decoder delivers: 'bgr' [..., IH, IW, 3 | 4], 'nv12' / 'i420' [..., IH*3/2, IW]
    (IH and IW even) or 'yuyv' [..., IH, IW, 2] (IW even), byte-linear per frame.  The four taps of an output pixel are converted
    as they are read -- chroma the nearest sample, the integer matrix `matrix` ('bt601' or 'bt709', limited range, or 'jfif', full
    range) of include/eve_hip.h eve_eye_warp_fmt_to_nchw -- so the result equals the 'rgb' call on the converted frame bit for
    bit, and no RGB frame is made.

    layout: None, or a SurfaceLayout: the frames are then surfaces as they lie in memory, uint8 [..., rows, pitch] or
    [..., frame_bytes] with the warps' leading dimensions, and the taps are read through the layout's address rule
    (eve_eye_warp_surface_to_nchw): the result equals the call on the de-pitched, cropped, byte-linear frame bit for bit.  `format`
    stays at its default (ValueError): the layout names it."""
    if layout is not None:
        if format != 'rgb':
            raise ValueError('warp_eye_patches: a layout names the format itself: leave format at its default')
        if not torch.is_tensor(warps) or warps.dim() < 3:
            raise TypeError('expected float32 warps shaped [..., 3, 3], got %s' % (tuple(getattr(warps, 'shape', ())),))
        flat, lead = surface_frames(frames, layout, warps.dim() - 2)
    elif format == 'rgb':
        flat, lead = _fold(frames)
        if flat.shape[3] not in (3, 4):
            raise TypeError('expected camera frames with 3 or 4 channels, got %d' % flat.shape[3])
    else:
        from .kernels import pixel_format_shape
        dims = 2 if format in ('nv12', 'i420') else 3          # the planar layouts are [rows, IW]
        if not torch.is_tensor(frames) or frames.dim() < dims + 1:
            raise TypeError('expected uint8 %s frames with at least one leading dimension, got %s' % (format, tuple(getattr(frames, 'shape', ()))))
        lead = tuple(frames.shape[:-dims])
        flat = frames.reshape((-1,) + tuple(frames.shape[-dims:])).contiguous()
        pixel_format_shape(flat, format, lead=1)
    if not torch.is_tensor(warps) or warps.dtype != torch.float32 or tuple(warps.shape) != lead + (3, 3):
        raise TypeError('expected float32 warps shaped %s, got %s %s' % (lead + (3, 3), getattr(warps, 'dtype', type(warps)),
                                                                         tuple(getattr(warps, 'shape', ()))))
    if lens is not None and (not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) != lead + (12,)):
        raise TypeError('expected float32 lens rows shaped %s, got %s %s' % (lead + (12,), getattr(lens, 'dtype', type(lens)),
                                                                             tuple(getattr(lens, 'shape', ()))))
    hw = eye_patch_hw() if size is None else (int(size[0]), int(size[1]))
    warps = warps.reshape(-1, 3, 3).contiguous()
    lens = None if lens is None else lens.reshape(-1, 12).contiguous()
    if layout is not None:
        out = default_kernels().eye_warp_surface_to_nchw(flat, warps, hw, layout, matrix=matrix, lens=lens)
    elif format != 'rgb':
        out = default_kernels().eye_warp_fmt_to_nchw(flat, warps, hw, format, matrix=matrix, lens=lens)
    elif lens is None:
        out = default_kernels().eye_warp_u8_to_nchw(flat, warps, hw)
    else:
        out = default_kernels().eye_warp_lens_u8_to_nchw(flat, warps, lens, hw)
    return out.view(lead + tuple(out.shape[1:]))


def quantise_patches(patches):
    """Float eye patches [..., 3, H, W] in [-1, 1] -> uint8 [..., H, W, 3]: clamp(rint((p + 1) * 127.5), 0, 255) in float32, the
    inverse of preprocess_frames on every value it produces."""
    q = torch.clamp(torch.round((patches.float() + 1.0) * 127.5), 0.0, 255.0).to(torch.uint8)
    return q.movedim(-3, -1).contiguous()


def _color(c, what):
    if isinstance(c, int):
        c = ((c >> 16) & 255, (c >> 8) & 255, c & 255) if 0 <= c <= 0xffffff else None
    if c is None or len(c) != 3 or not all(isinstance(v, (int, np.integer)) and 0 <= int(v) <= 255 for v in c):
        raise ValueError('%s must be (r, g, b) with values in 0..255 or 0xRRGGBB' % what)
    return tuple(int(v) for v in c)


class OverlaySpec(object):
    """What EVEStream.step(chunk, render=spec) draws onto the chunk's full-resolution screen capture (eve_overlay_render).
      out_format   'nv12' (default, what a hardware encoder reads), 'i420', 'rgb' or 'bgr'
      matrix       the matrix of the output, 'bt601' | 'bt709' | 'jfif'; None: the capture's (model.refine_net.yuv_matrix)
      markers      a list of dicts: key -- a [B, Tc, 2] entry of the step's result or of the chunk, in actual_screen_size pixels
                   ('PoG_px_initial', 'PoG_px_final', a caller's 'PoG_px_gt'); valid -- None or the key of a [B, Tc] bool / uint8
                   entry; r_fill, r_outline -- radii in output pixels, 0..255; fill, outline -- (r, g, b) or 0xRRGGBB.  At most 8,
                   drawn in list order.  The default is the reference's look at 1080p: the initial estimate (180, 180, 0), then the
                   refined one (0, 180, 0), radii 10 / 14, a black outline.
      heat         True: blend heatmap_final in heat_color (default red) up to alpha heat_amax (0..255, default 128)
      heat_key     None, or the name of a per_frame=True GazeHistorySpec of the same step (history=...): that map's frame is blended
                   in place of heatmap_final (axes up to 1024; not together with heat=True)
      inset        None, 'eyes' (the step's eye patches as [right | left]) or the key of a uint8 [B, Tc, h, w, 3] RGB chunk entry;
                   inset_xy (x0, y0) of its top-left pixel, None: flush in the bottom-right corner; inset_zoom 1..4 (nearest);
                   inset_mirror (default True, as the reference shows the eyes)
    Instances compare and hash by value: the spec is part of a captured graph's key."""
    DEFAULT_MARKERS = (dict(key='PoG_px_initial', fill=(180, 180, 0)), dict(key='PoG_px_final', fill=(0, 180, 0)))

    def __init__(self, out_format='nv12', matrix=None, markers=DEFAULT_MARKERS, heat=False, heat_color=(255, 0, 0), heat_amax=128,
                 inset='eyes', inset_xy=None, inset_zoom=1, inset_mirror=True, heat_key=None):
        from .kernels import OVERLAY_MAX_MARKERS, OVERLAY_OUT_FORMATS, YUV_MATRICES
        if out_format not in OVERLAY_OUT_FORMATS:
            raise ValueError('OverlaySpec: out_format must be rgb, bgr, nv12 or i420, got %r' % (out_format,))
        if matrix is not None and matrix not in YUV_MATRICES:
            raise ValueError('OverlaySpec: matrix must be None or one of %s, got %r' % (', '.join(YUV_MATRICES), matrix))
        markers = list(markers or ())
        if len(markers) > OVERLAY_MAX_MARKERS:
            raise ValueError('OverlaySpec: markers holds %d entries, at most %d are drawn' % (len(markers), OVERLAY_MAX_MARKERS))
        rows = []
        for i, m in enumerate(markers):
            unknown = set(m) - {'key', 'valid', 'r_fill', 'r_outline', 'fill', 'outline'}
            if unknown or 'key' not in m:
                raise ValueError('OverlaySpec: markers[%d] needs key and may hold valid, r_fill, r_outline, fill, outline; got %s' % (i, sorted(m)))
            r_fill, r_out = int(m.get('r_fill', 10)), int(m.get('r_outline', 14))
            if not (0 <= r_fill <= 255 and 0 <= r_out <= 255):
                raise ValueError('OverlaySpec: markers[%d] radii must be in 0..255' % i)
            rows.append((str(m['key']), None if m.get('valid') is None else str(m['valid']), r_fill, r_out,
                         _color(m.get('fill', (0, 180, 0)), 'OverlaySpec: markers[%d] fill' % i),
                         _color(m.get('outline', (0, 0, 0)), 'OverlaySpec: markers[%d] outline' % i)))
        if not 0 <= int(heat_amax) <= 255:
            raise ValueError('OverlaySpec: heat_amax must be in 0..255, got %r' % (heat_amax,))
        if heat_key is not None and (not isinstance(heat_key, str) or not heat_key):
            raise ValueError('OverlaySpec: heat_key must be None or the name of a per_frame GazeHistorySpec, got %r' % (heat_key,))
        if heat_key is not None and heat:
            raise ValueError('OverlaySpec: heat_key blends a gaze history map in place of heatmap_final: not together with heat=True')
        if inset is not None and not isinstance(inset, str):
            raise ValueError("OverlaySpec: inset must be None, 'eyes' or the key of a uint8 [B, Tc, h, w, 3] chunk entry")
        if not 1 <= int(inset_zoom) <= 4:
            raise ValueError('OverlaySpec: inset_zoom must be in 1..4, got %r' % (inset_zoom,))
        self.out_format, self.matrix, self.markers = out_format, matrix, tuple(rows)
        self.heat, self.heat_color, self.heat_amax = bool(heat), _color(heat_color, 'OverlaySpec: heat_color'), int(heat_amax)
        self.inset, self.inset_zoom, self.inset_mirror = inset, int(inset_zoom), bool(inset_mirror)
        self.inset_xy = None if inset_xy is None else (int(inset_xy[0]), int(inset_xy[1]))
        self.heat_key = heat_key

    def key(self):
        return (self.out_format, self.matrix, self.markers, self.heat, self.heat_color, self.heat_amax, self.inset, self.inset_xy,
                self.inset_zoom, self.inset_mirror, self.heat_key)

    def __eq__(self, other):
        return isinstance(other, OverlaySpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def marker_table(self):
        """-> the int32 [M, 4] rows (r_fill, r_outline, fill 0xRRGGBB, outline 0xRRGGBB) of eve_overlay_render, as nested lists."""
        rgb = lambda c: (c[0] << 16) | (c[1] << 8) | c[2]
        return [[r_fill, r_out, rgb(fill), rgb(outline)] for _, _, r_fill, r_out, fill, outline in self.markers]


GAZE_EVENT_KEYS = ('PoG_px_filtered', 'gaze_velocity', 'gaze_event', 'fixation_id', 'fixation_px', 'fixation_ms', 'fixating')
GAZE_EVENT_SOURCES = ('PoG_px_initial', 'PoG_px_final')


class GazeEventSpec(object):
    """What EVEStream.step(chunk, events=spec) adds at the end of the step (eve_gaze_events): the point of gaze smoothed by a one-euro
    filter, the angular gaze velocity, fixation / saccade labels by a velocity threshold (I-VT), the running fixation, and completed
    fixations in the EVEStream's store.
      source           'PoG_px_initial', 'PoG_px_final' (needs a RefineNet) or None: PoG_px_final with a RefineNet, else PoG_px_initial
      fps              frames per second of the streams, for chunks without frame_time (float64 [B, Tc] seconds, which wins when
                       both are there): frame i since the stream's last reset then has t = i / fps
      min_cutoff_hz, beta, d_cutoff_hz   the one-euro filter's parameters, on pixels and pixels / second
      velocity_from    'filtered' (default) or 'raw': the point of gaze behind the velocity
      saccade_deg_s    above this angular velocity (degrees / second) a frame is a saccade (2), else a fixation (1)
      min_fixation_s   a fixation counts (`fixating`, the store) once it has lasted this long
      max_gap_s        two samples further apart than this are not connected: the filter and the fixation start afresh
    Instances compare and hash by value: the spec is part of a captured graph's key.  Not offered: dispersion (I-DT) or other
    classifiers, windowed velocity, merging of adjacent fixations and retroactive relabelling, a blink class, per-eye events,
    gradients, EVE.forward.  (Smooth pursuit, the third class, and its windowed velocity: PursuitSpec.)"""

    def __init__(self, source=None, fps=None, min_cutoff_hz=1.0, beta=0.007, d_cutoff_hz=1.0, velocity_from='filtered', saccade_deg_s=30.0,
                 min_fixation_s=0.06, max_gap_s=0.075):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        if source is not None and source not in GAZE_EVENT_SOURCES:
            raise ValueError('GazeEventSpec: source must be None or one of %s, got %r' % (', '.join(GAZE_EVENT_SOURCES), source))
        if velocity_from not in ('filtered', 'raw'):
            raise ValueError("GazeEventSpec: velocity_from must be 'filtered' or 'raw', got %r" % (velocity_from,))
        values = {'min_cutoff_hz': min_cutoff_hz, 'd_cutoff_hz': d_cutoff_hz, 'saccade_deg_s': saccade_deg_s, 'min_fixation_s': min_fixation_s,
                  'max_gap_s': max_gap_s}
        if fps is not None:
            values['fps'] = fps
        for name, v in values.items():
            if not number(v) or not v > 0:
                raise ValueError('GazeEventSpec: %s must be a finite number > 0, got %r' % (name, v))
        if not number(beta) or beta < 0:
            raise ValueError('GazeEventSpec: beta must be a finite number >= 0, got %r' % (beta,))
        self.source, self.velocity_from = source, velocity_from
        self.fps = None if fps is None else float(fps)
        self.min_cutoff_hz, self.beta, self.d_cutoff_hz = float(min_cutoff_hz), float(beta), float(d_cutoff_hz)
        self.saccade_deg_s, self.min_fixation_s, self.max_gap_s = float(saccade_deg_s), float(min_fixation_s), float(max_gap_s)

    def key(self):
        return (self.source, self.fps, self.min_cutoff_hz, self.beta, self.d_cutoff_hz, self.velocity_from, self.saccade_deg_s,
                self.min_fixation_s, self.max_gap_s)

    def __eq__(self, other):
        return isinstance(other, GazeEventSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'GazeEventSpec(source=%r, fps=%r, min_cutoff_hz=%r, beta=%r, d_cutoff_hz=%r, velocity_from=%r, saccade_deg_s=%r, ' \
               'min_fixation_s=%r, max_gap_s=%r)' % self.key()


def gaze_events(pog_px, o, inv_camera_transformation, pixels_per_millimeter, spec, frame_time=None, valid=None, fixation_capacity=256):
    """The gaze filter and the fixation / saccade events of S recorded streams, stand-alone and from fresh state: pog_px float32
    [S, T, 2] (actual_screen_size pixels), o [S, T, 3] (the binocular origin), inv_camera_transformation [S, T, 4, 4],
    pixels_per_millimeter [S, T, 2], device tensors; spec a GazeEventSpec (its source is not looked at); frame_time None (then
    spec.fps) or float64 [S, T] seconds; valid None or bool / uint8 [S, T].  One eve_gaze_events launch, which also closes the
    fixations still open at the clip's end.  -> the seven per-frame keys of EVEStream.step(events=...) plus fixations (float64
    [S, fixation_capacity, 8], rows (id, t_start, t_last, n, cx, cy, rms_px, 0)), fixation_count and fixation_dropped (int32 [S]);
    the host does not wait.  Not offered: dispersion classifiers, windowed velocity, merging of adjacent fixations, a blink class,
    per-eye events, gradients.  (Smooth pursuit: gaze_pursuits.)"""
    if not isinstance(spec, GazeEventSpec):
        raise ValueError('gaze_events: spec must be an eve_amd.GazeEventSpec, got %s' % type(spec).__name__)
    if not torch.is_tensor(pog_px) or pog_px.dtype != torch.float32 or pog_px.dim() != 3 or pog_px.shape[2] != 2 or pog_px.numel() == 0:
        raise TypeError('gaze_events: pog_px must be float32 [S, T, 2], got %s %s' % (getattr(pog_px, 'dtype', type(pog_px)),
                                                                                     tuple(getattr(pog_px, 'shape', ()))))
    S, T = pog_px.shape[:2]
    for name, t, shape in (('o', o, (S, T, 3)), ('inv_camera_transformation', inv_camera_transformation, (S, T, 4, 4)),
                           ('pixels_per_millimeter', pixels_per_millimeter, (S, T, 2))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise TypeError('gaze_events: %s must be float32 %s, got %s %s' % (name, list(shape), getattr(t, 'dtype', type(t)),
                                                                              tuple(getattr(t, 'shape', ()))))
    if frame_time is None and spec.fps is None:
        raise ValueError('gaze_events: frame_time, or a spec with fps')
    if frame_time is not None and (not torch.is_tensor(frame_time) or frame_time.dtype != torch.float64 or tuple(frame_time.shape) != (S, T)):
        raise TypeError('gaze_events: frame_time must be float64 [%d, %d] seconds' % (S, T))
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (S, T):
            raise TypeError('gaze_events: valid must be bool or uint8 [%d, %d]' % (S, T))
        valid = valid.contiguous()
        valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
    if isinstance(fixation_capacity, bool) or not isinstance(fixation_capacity, int) or fixation_capacity < 1:
        raise ValueError('gaze_events: fixation_capacity must be an integer >= 1, got %r' % (fixation_capacity,))
    dev = pog_px.device
    state = torch.zeros((S, 32), dtype=torch.float64, device=dev)
    store = torch.zeros((S, fixation_capacity, 8), dtype=torch.float64, device=dev)
    count, dropped = torch.zeros((S,), dtype=torch.int32, device=dev), torch.zeros((S,), dtype=torch.int32, device=dev)
    out = default_kernels().gaze_events(pog_px.contiguous(), o.contiguous(), inv_camera_transformation.contiguous(),
                                        pixels_per_millimeter.contiguous(), spec, state, store, count, dropped,
                                        frame_time=None if frame_time is None else frame_time.contiguous(), valid=valid,
                                        flush=torch.ones((S,), dtype=torch.int32, device=dev))
    out = dict(out)
    out.update(fixations=store, fixation_count=count, fixation_dropped=dropped)
    return out


SACCADE_KEYS = ('saccade_id', 'saccade_ms')      # the per-frame results of the saccade stage
SACCADE_STATE = 32                               # doubles per stream of eve_gaze_saccades' state row
SACCADE_ROW = 16                                 # ... of its table row and of a stored saccade
SACCADE_COLUMNS = ('id', 't_onset', 't_landing', 'n', 'x0', 'y0', 'x1', 'y1', 'amplitude_deg', 'peak_deg_s', 'mean_deg_s',
                   'prev_fixation_id', 'next_fixation_id', 'missing')
SACCADE_TABLE = ('accepted', 'sum_amp', 'sum_amp2', 'sum_peak', 'sum_amp_peak', 'sum_dur', 'sum_amp_dur', 'max_amp', 'max_peak', 'aborted',
                 'small', 'short', 'long', 'interrupted')


class SaccadeSpec(object):
    """What EVEStream.step(chunk, events=..., saccades=spec) adds after the events stage (eve_gaze_saccades): the runs of saccade frames
    become events with amplitude, duration, peak and mean velocity and the ids of the fixations on either side, in the EVEStream's
    store, with a table of tallies (the sums behind the main sequence: main_sequence()).
      min_amplitude_deg   a saccade whose onset and landing gaze vectors are less than this apart is tallied `small` and not stored
      min_duration_s      one shorter than this (onset to landing) is tallied `short`
      max_duration_s      one longer than this is tallied `long` (0.2 s: above any physiological saccade)
      max_missing         one with more frames that were no sample inside it is tallied `interrupted`
    The amplitude is that of the point the velocity is from: with GazeEventSpec(velocity_from='filtered'), the default, the
    one-euro filter's lag shortens it; 'raw' gives the source's.  Instances compare and hash by value: the spec is part of a captured
    graph's key.  Not offered: direction angles (the endpoints are there), curvature or path length, glissades and post-saccadic
    oscillation, microsaccades, per-eye saccades, retroactive merging, gradients, EVE.forward.  (Smooth pursuit: PursuitSpec.)"""

    def __init__(self, min_amplitude_deg=0.5, min_duration_s=0.0, max_duration_s=0.2, max_missing=0):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        for name, v in (('min_amplitude_deg', min_amplitude_deg), ('min_duration_s', min_duration_s)):
            if not number(v) or v < 0:
                raise ValueError('SaccadeSpec: %s must be a finite number >= 0, got %r' % (name, v))
        if not number(max_duration_s) or not max_duration_s > 0:
            raise ValueError('SaccadeSpec: max_duration_s must be a finite number > 0, got %r' % (max_duration_s,))
        if isinstance(max_missing, bool) or not isinstance(max_missing, (int, np.integer)) or not 0 <= max_missing <= 0x7fffffff:
            raise ValueError('SaccadeSpec: max_missing must be an integer >= 0, got %r' % (max_missing,))
        self.min_amplitude_deg, self.min_duration_s, self.max_duration_s = float(min_amplitude_deg), float(min_duration_s), float(max_duration_s)
        self.max_missing = int(max_missing)

    def key(self):
        return (self.min_amplitude_deg, self.min_duration_s, self.max_duration_s, self.max_missing)

    def __eq__(self, other):
        return isinstance(other, SaccadeSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'SaccadeSpec(min_amplitude_deg=%r, min_duration_s=%r, max_duration_s=%r, max_missing=%r)' % self.key()


def saccade_buffers(S, capacity, device):
    """-> (state float64 [S, 32], table float64 [S, 16], store float64 [S, capacity, 16], count and dropped int32 [S]) of S streams
    that have seen nothing: what eve_gaze_saccades carries (include/eve_hip.h has the rows)."""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)
    return (z((S, SACCADE_STATE), torch.float64), z((S, SACCADE_ROW), torch.float64), z((S, capacity, SACCADE_ROW), torch.float64),
            z((S,), torch.int32), z((S,), torch.int32))


def saccade_stage(k, pog, res, spec, saccade_spec, buffers, lengths=None, reset=None):
    """The one eve_gaze_saccades launch behind EVEStream.step and gaze_saccades: k the kernels, pog the events' source point [B, T, 2],
    res gaze_events_ex's result, buffers the five carried tensors -> the two per-frame keys.  The point is the one the velocity is
    from."""
    point = pog if spec.velocity_from == 'raw' else res['PoG_px_filtered']
    return k.gaze_saccades(res['sample'], res['sample_time'], res['gaze_vector'], point, res['gaze_event'], res['gaze_velocity'],
                           res['fixation_id'], saccade_spec, *buffers, lengths=lengths, reset=reset)


def gaze_saccades(pog_px, o, inv_camera_transformation, pixels_per_millimeter, spec, saccade_spec, frame_time=None, valid=None,
                  saccade_capacity=256):
    """The fixation / saccade events AND the saccades of S recorded streams, stand-alone and from fresh state: gaze_events' arguments
    (spec a GazeEventSpec) plus saccade_spec, a SaccadeSpec.  One eve_gaze_events_ex and one eve_gaze_saccades launch.  -> the seven
    per-frame keys of the events, saccade_id int32 [S, T] (-1 outside a saccade) and saccade_ms float32 [S, T], plus saccades
    (float64 [S, saccade_capacity, 16], rows SACCADE_COLUMNS: id, t_onset, t_landing, n, x0, y0, x1, y1, amplitude_deg, peak_deg_s,
    mean_deg_s, prev_fixation_id, next_fixation_id, missing, 0, 0), saccade_count and saccade_dropped (int32 [S]) and saccade_table
    (float64 [S, 16], entries SACCADE_TABLE; main_sequence() reads it); the host does not wait.  A saccade still open at the clip's
    end has no landing and is not stored.  Not offered: see SaccadeSpec."""
    if not isinstance(spec, GazeEventSpec):
        raise ValueError('gaze_saccades: spec must be an eve_amd.GazeEventSpec, got %s' % type(spec).__name__)
    if not isinstance(saccade_spec, SaccadeSpec):
        raise ValueError('gaze_saccades: saccade_spec must be an eve_amd.SaccadeSpec, got %s' % type(saccade_spec).__name__)
    if not torch.is_tensor(pog_px) or pog_px.dtype != torch.float32 or pog_px.dim() != 3 or pog_px.shape[2] != 2 or pog_px.numel() == 0:
        raise TypeError('gaze_saccades: pog_px must be float32 [S, T, 2], got %s %s' % (getattr(pog_px, 'dtype', type(pog_px)),
                                                                                       tuple(getattr(pog_px, 'shape', ()))))
    S, T = pog_px.shape[:2]
    for name, t, shape in (('o', o, (S, T, 3)), ('inv_camera_transformation', inv_camera_transformation, (S, T, 4, 4)),
                           ('pixels_per_millimeter', pixels_per_millimeter, (S, T, 2))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise TypeError('gaze_saccades: %s must be float32 %s, got %s %s' % (name, list(shape), getattr(t, 'dtype', type(t)),
                                                                                tuple(getattr(t, 'shape', ()))))
    if frame_time is None and spec.fps is None:
        raise ValueError('gaze_saccades: frame_time, or a spec with fps')
    if frame_time is not None and (not torch.is_tensor(frame_time) or frame_time.dtype != torch.float64 or tuple(frame_time.shape) != (S, T)):
        raise TypeError('gaze_saccades: frame_time must be float64 [%d, %d] seconds' % (S, T))
    if valid is not None:
        valid = _bool_rows(valid, (S, T), 'gaze_saccades: valid')
    if isinstance(saccade_capacity, bool) or not isinstance(saccade_capacity, (int, np.integer)) or saccade_capacity < 1:
        raise ValueError('gaze_saccades: saccade_capacity must be an integer >= 1, got %r' % (saccade_capacity,))
    dev = pog_px.device
    k = default_kernels()
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    pog_px = pog_px.contiguous()
    # (the fixation store is not returned -- gaze_events has it -- so one row per stream does)
    res = k.gaze_events_ex(pog_px, o.contiguous(), inv_camera_transformation.contiguous(), pixels_per_millimeter.contiguous(), spec,
                           z((S, 32), torch.float64), z((S, 1, 8), torch.float64), z((S,), torch.int32), z((S,), torch.int32),
                           frame_time=None if frame_time is None else frame_time.contiguous(), valid=valid)
    buffers = saccade_buffers(S, int(saccade_capacity), dev)
    out = {k_: res[k_] for k_ in GAZE_EVENT_KEYS}
    out.update(saccade_stage(k, pog_px, res, spec, saccade_spec, buffers))
    out.update(saccades=buffers[2], saccade_count=buffers[3], saccade_dropped=buffers[4], saccade_table=buffers[1])
    return out


def main_sequence(table):
    """The main sequence from the saccade table's sums, on the host in numpy: table float64 [S, 16] or [16] (EVEStream.saccade_table(),
    gaze_saccades()['saccade_table']; a tensor is copied to the host, which waits) -> a dict of float64 [S] (or scalars): n, the two
    least-squares lines duration_s = duration_intercept + duration_slope * amplitude_deg and peak_deg_s = peak_intercept + peak_slope *
    amplitude_deg over the accepted saccades, mean_amplitude_deg, max_amplitude_deg and max_peak_deg_s.  The four coefficients are NaN
    with fewer than 2 saccades or no spread in amplitude."""
    t = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    t = np.asarray(t, dtype=np.float64)
    if t.shape[-1:] != (SACCADE_ROW,) or t.ndim not in (1, 2):
        raise ValueError('main_sequence: table must be [S, 16] or [16], got %s' % (t.shape,))
    n, sa, saa, sp, sap, sd, sad = (t[..., i] for i in range(7))
    with np.errstate(all='ignore'):
        det = n * saa - sa * sa
        good = (n >= 2) & (det > 1e-12 * (n * saa))      # (equal amplitudes leave rounding noise, not a spread)
        det = np.where(good, det, np.nan)
        d_slope, p_slope = (n * sad - sa * sd) / det, (n * sap - sa * sp) / det
        out = {'n': n.copy(), 'duration_slope': d_slope, 'duration_intercept': (sd - d_slope * sa) / n, 'peak_slope': p_slope,
               'peak_intercept': (sp - p_slope * sa) / n, 'mean_amplitude_deg': np.where(n > 0, sa / n, np.nan),
               'max_amplitude_deg': t[..., 7].copy(), 'max_peak_deg_s': t[..., 8].copy()}
    return out


PURSUIT_KEYS = ('gaze_class', 'pursuit_id', 'pursuit_ms', 'gaze_velocity_windowed', 'gaze_straightness', 'pursuit_gain')
PURSUIT_STATE = 320                              # doubles per stream of eve_gaze_pursuits' state row: 32 scalars + 32 ring entries of 9
PURSUIT_TABLE_ROW = 16                           # ... of its table row
PURSUIT_ROW = 20                                 # ... of a stored episode
PURSUIT_COLUMNS = ('id', 't_onset', 't_end', 'n', 'x0', 'y0', 'x1', 'y1', 'amplitude_deg', 'direction_deg', 'mean_deg_s', 'peak_deg_s',
                   'path_deg', 'fixation_id', 'missing', 'gain_n', 'mean_gain', 'mean_error_px')
PURSUIT_TABLE = ('accepted', 'sum_dur', 'sum_amp', 'sum_path', 'sum_mean_v', 'max_peak', 'sum_gain', 'gain_n', 'aborted', 'small', 'short',
                 'interrupted')


class PursuitSpec(object):
    """What EVEStream.step(chunk, events=..., pursuits=spec) adds after the events (and the saccade) stage (eve_gaze_pursuits): smooth
    pursuit as the third gaze class.  Each fixation-labelled sample is looked at over a window of the chained samples before it; where
    the gaze turned steadily and straight the frame is promoted to the pursuit class (gaze_class 3), and the runs of such frames
    become episodes with amplitude, direction, mean and peak velocity, path length and -- with pursuit_target in the chunk -- gain and
    position error, in the EVEStream's store, with a table of tallies (pursuit_summary()).
      window_s            the window: the chained fixation samples of the last window_s seconds, at most 32 of them
      min_window_s        a window shorter than this (after a saccade, a gap, a reset) decides nothing; <= window_s
      pursuit_deg_s       the angle between the window's first and last gaze vector, over its time, must reach this (degrees / second)
      min_straightness    ... and that angle over the window's path length (the sum of the events' velocities times their steps) this,
                          in (0, 1]: fixational jitter wanders, pursuit goes straight
      settle_s            the fixation samples this soon after a saccade frame stay out of the windows (the filter's creep after a landing)
      min_duration_s      an episode shorter than this (onset to last sample) is tallied `short` and not stored
      min_amplitude_deg   one whose onset and last gaze vectors are less than this apart is tallied `small`
      max_missing         one with more frames that were no sample inside it is tallied `interrupted`
    Pursuit wants the filtered point (GazeEventSpec(velocity_from='filtered'), the default): with 'raw', jitter lowers the
    straightness and fragments the episodes at high frame rates (tests/pursuit_ref.py on an 8 degrees / second ramp with 0.1 degrees
    of jitter at 120 fps: 8 fragments raw, 3 of them accepted and 5 short; one episode when filtered).  Instances compare and hash by value: the spec is part of a captured graph's key.  Not offered: hysteresis, or
    merging episodes across catch-up saccades (the rows carry what a host merge needs: times, endpoints, the fixation id);
    retroactive relabelling of the frames before a window fills; per-eye pursuit; vestibulo-ocular compensation; gradients;
    EVE.forward."""

    def __init__(self, window_s=0.2, min_window_s=0.1, pursuit_deg_s=3.0, min_straightness=0.7, settle_s=0.08, min_duration_s=0.15,
                 min_amplitude_deg=1.0, max_missing=3):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        for name, v in (('window_s', window_s), ('min_window_s', min_window_s), ('pursuit_deg_s', pursuit_deg_s)):
            if not number(v) or not v > 0:
                raise ValueError('PursuitSpec: %s must be a finite number > 0, got %r' % (name, v))
        if min_window_s > window_s:
            raise ValueError('PursuitSpec: min_window_s must be <= window_s (%r), got %r' % (window_s, min_window_s))
        if not number(min_straightness) or not 0 < min_straightness <= 1:
            raise ValueError('PursuitSpec: min_straightness must lie in (0, 1], got %r' % (min_straightness,))
        for name, v in (('settle_s', settle_s), ('min_duration_s', min_duration_s), ('min_amplitude_deg', min_amplitude_deg)):
            if not number(v) or v < 0:
                raise ValueError('PursuitSpec: %s must be a finite number >= 0, got %r' % (name, v))
        if isinstance(max_missing, bool) or not isinstance(max_missing, (int, np.integer)) or not 0 <= max_missing <= 0x7fffffff:
            raise ValueError('PursuitSpec: max_missing must be an integer >= 0, got %r' % (max_missing,))
        self.window_s, self.min_window_s, self.pursuit_deg_s = float(window_s), float(min_window_s), float(pursuit_deg_s)
        self.min_straightness, self.settle_s, self.min_duration_s = float(min_straightness), float(settle_s), float(min_duration_s)
        self.min_amplitude_deg, self.max_missing = float(min_amplitude_deg), int(max_missing)

    def key(self):
        return (self.window_s, self.min_window_s, self.pursuit_deg_s, self.min_straightness, self.settle_s, self.min_duration_s,
                self.min_amplitude_deg, self.max_missing)

    def __eq__(self, other):
        return isinstance(other, PursuitSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'PursuitSpec(window_s=%r, min_window_s=%r, pursuit_deg_s=%r, min_straightness=%r, settle_s=%r, min_duration_s=%r, ' \
               'min_amplitude_deg=%r, max_missing=%r)' % self.key()


def pursuit_buffers(S, capacity, device):
    """-> (state float64 [S, 320], table float64 [S, 16], store float64 [S, capacity, 20], count and dropped int32 [S]) of S streams
    that have seen nothing: what eve_gaze_pursuits carries (include/eve_hip.h has the rows)."""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)
    return (z((S, PURSUIT_STATE), torch.float64), z((S, PURSUIT_TABLE_ROW), torch.float64), z((S, capacity, PURSUIT_ROW), torch.float64),
            z((S,), torch.int32), z((S,), torch.int32))


def pursuit_stage(k, pog, res, spec, pursuit_spec, buffers, target=None, lengths=None, reset=None):
    """The one eve_gaze_pursuits launch behind EVEStream.step and gaze_pursuits: k the kernels, pog the events' source point [B, T, 2],
    res gaze_events_ex's result, buffers the five carried tensors, target float32 [B, T, 2] or None -> the six per-frame keys.  The
    point is the one the velocity is from, as for saccade_stage."""
    point = pog if spec.velocity_from == 'raw' else res['PoG_px_filtered']
    return k.gaze_pursuits(res['sample'], res['sample_time'], res['gaze_vector'], point, res['gaze_event'], res['gaze_velocity'],
                           res['fixation_id'], pursuit_spec, *buffers, target=target, lengths=lengths, reset=reset)


def gaze_pursuits(pog_px, o, inv_camera_transformation, pixels_per_millimeter, spec, pursuit_spec, frame_time=None, valid=None, target=None,
                  pursuit_capacity=256):
    """The fixation / saccade events AND the smooth pursuit of S recorded streams, stand-alone and from fresh state: gaze_events'
    arguments (spec a GazeEventSpec) plus pursuit_spec, a PursuitSpec, and target, None or float32 [S, T, 2] (the pursued object's
    screen position in pixels, NaN where there is none).  One eve_gaze_events_ex and one eve_gaze_pursuits launch.  -> the seven
    per-frame keys of the events (unchanged: the pursuit frames are still fixation frames there), gaze_class uint8 [S, T] (0 none, 1
    fixation, 2 saccade, 3 pursuit), pursuit_id int32 [S, T] (-1 outside an episode), pursuit_ms, gaze_velocity_windowed,
    gaze_straightness and pursuit_gain float32 [S, T] (the last three NaN where undefined), plus pursuits (float64 [S,
    pursuit_capacity, 20], rows PURSUIT_COLUMNS: id, t_onset, t_end, n, x0, y0, x1, y1, amplitude_deg, direction_deg (screen axes, y
    down), mean_deg_s, peak_deg_s, path_deg, fixation_id, missing, gain_n, mean_gain, mean_error_px, 0, 0), pursuit_count and
    pursuit_dropped (int32 [S]) and pursuit_table (float64 [S, 16], entries PURSUIT_TABLE; pursuit_summary() reads it); the host does
    not wait.  An episode still open at the clip's end is not stored.  Not offered: see PursuitSpec."""
    if not isinstance(spec, GazeEventSpec):
        raise ValueError('gaze_pursuits: spec must be an eve_amd.GazeEventSpec, got %s' % type(spec).__name__)
    if not isinstance(pursuit_spec, PursuitSpec):
        raise ValueError('gaze_pursuits: pursuit_spec must be an eve_amd.PursuitSpec, got %s' % type(pursuit_spec).__name__)
    if not torch.is_tensor(pog_px) or pog_px.dtype != torch.float32 or pog_px.dim() != 3 or pog_px.shape[2] != 2 or pog_px.numel() == 0:
        raise TypeError('gaze_pursuits: pog_px must be float32 [S, T, 2], got %s %s' % (getattr(pog_px, 'dtype', type(pog_px)),
                                                                                       tuple(getattr(pog_px, 'shape', ()))))
    S, T = pog_px.shape[:2]
    for name, t, shape in (('o', o, (S, T, 3)), ('inv_camera_transformation', inv_camera_transformation, (S, T, 4, 4)),
                           ('pixels_per_millimeter', pixels_per_millimeter, (S, T, 2))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise TypeError('gaze_pursuits: %s must be float32 %s, got %s %s' % (name, list(shape), getattr(t, 'dtype', type(t)),
                                                                                tuple(getattr(t, 'shape', ()))))
    if target is not None and (not torch.is_tensor(target) or target.dtype != torch.float32 or tuple(target.shape) != (S, T, 2)):
        raise TypeError('gaze_pursuits: target must be float32 [%d, %d, 2], got %s %s' % (S, T, getattr(target, 'dtype', type(target)),
                                                                                         tuple(getattr(target, 'shape', ()))))
    if frame_time is None and spec.fps is None:
        raise ValueError('gaze_pursuits: frame_time, or a spec with fps')
    if frame_time is not None and (not torch.is_tensor(frame_time) or frame_time.dtype != torch.float64 or tuple(frame_time.shape) != (S, T)):
        raise TypeError('gaze_pursuits: frame_time must be float64 [%d, %d] seconds' % (S, T))
    if valid is not None:
        valid = _bool_rows(valid, (S, T), 'gaze_pursuits: valid')
    if isinstance(pursuit_capacity, bool) or not isinstance(pursuit_capacity, (int, np.integer)) or pursuit_capacity < 1:
        raise ValueError('gaze_pursuits: pursuit_capacity must be an integer >= 1, got %r' % (pursuit_capacity,))
    dev = pog_px.device
    k = default_kernels()
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    pog_px = pog_px.contiguous()
    # (the fixation store is not returned -- gaze_events has it -- so one row per stream does)
    res = k.gaze_events_ex(pog_px, o.contiguous(), inv_camera_transformation.contiguous(), pixels_per_millimeter.contiguous(), spec,
                           z((S, 32), torch.float64), z((S, 1, 8), torch.float64), z((S,), torch.int32), z((S,), torch.int32),
                           frame_time=None if frame_time is None else frame_time.contiguous(), valid=valid)
    buffers = pursuit_buffers(S, int(pursuit_capacity), dev)
    out = {k_: res[k_] for k_ in GAZE_EVENT_KEYS}
    out.update(pursuit_stage(k, pog_px, res, spec, pursuit_spec, buffers, target=None if target is None else target.contiguous()))
    out.update(pursuits=buffers[2], pursuit_count=buffers[3], pursuit_dropped=buffers[4], pursuit_table=buffers[1])
    return out


def pursuit_summary(table):
    """The pursuit table's sums as means, on the host in numpy: table float64 [S, 16] or [16] (EVEStream.pursuit_table(),
    gaze_pursuits()['pursuit_table']; a tensor is copied to the host, which waits) -> a dict of float64 [S] (or scalars): n (the
    accepted episodes), pursuit_s (their total duration in seconds), mean_deg_s (the mean of the episodes' mean velocities), mean_gain
    (over the samples with a defined gain) and max_peak_deg_s.  The two means are NaN where there is nothing to average."""
    t = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    t = np.asarray(t, dtype=np.float64)
    if t.shape[-1:] != (PURSUIT_TABLE_ROW,) or t.ndim not in (1, 2):
        raise ValueError('pursuit_summary: table must be [S, 16] or [16], got %s' % (t.shape,))
    n, gain_n = t[..., 0], t[..., 7]
    with np.errstate(all='ignore'):
        return {'n': n.copy(), 'pursuit_s': t[..., 1].copy(), 'mean_deg_s': np.where(n > 0, t[..., 4] / n, np.nan),
                'mean_gain': np.where(gain_n > 0, t[..., 6] / gain_n, np.nan), 'max_peak_deg_s': t[..., 5].copy()}


GAZE_HISTORY_SOURCES = ('PoG_px_initial', 'PoG_px_final', 'PoG_px_filtered', 'fixation_px', 'heatmap_final')
GAZE_HISTORY_MAX_AXIS = 2048


class GazeHistorySpec(object):
    """What EVEStream.step(chunk, history=spec) adds to the step (eve_gaze_history_plan + eve_gaze_history_update): the time-decayed
    history of the point of gaze -- per stream the map M_t = decay_per_ms^(ms since the previous frame) * M_{t-1} + w_t * G_t, which is
    the reference's windowed sum (its initial_gaze_history / refined_gaze_history) as a recurrence, carried from step to step.
      name            the result key: <name> float32 [B, MH, MW], and with per_frame <name>_frames float32 [B, Tc, MH, MW]
      source          'PoG_px_initial', 'PoG_px_final', 'PoG_px_filtered', 'fixation_px' (the last two need events= in the same step),
                      'heatmap_final' (the network's own maps: needs a RefineNet and size == gaze_heatmap_size), or None: PoG_px_final
                      with a RefineNet, else PoG_px_initial
      valid_key       None or the key of a bool / uint8 [B, Tc] entry of the result or the chunk, ANDed into the frame's usability
                      (source='fixation_px', valid_key='fixating': the fixation heat map)
      size            (MW, MH), each 1 .. 2048; None: config.gaze_heatmap_size
      sigma           of the Gaussian, in map pixels, > 0; None: config.gaze_heatmap_sigma_history
      decay_per_ms    in (0, 1]; None: config.gaze_history_map_decay_per_ms; 1.0: no decay
      weight          'frame': every usable frame deposits 1 (the reference's); 'seconds': the time since the previous tick, capped by
                      max_gap_s (with decay_per_ms=1: a dwell map in seconds)
      fps             for chunks without frame_time (float64 [B, Tc] seconds, which wins when both are there)
      floor           added to every Gaussian; 1e-8 reproduces the reference's maps
      normalize       True: every deposit times 1 / (2 pi sigma^2), so the map integrates to the weight deposited
      per_frame       True: also the map after every frame
    Instances compare and hash by value: the spec is part of a captured graph's key, and a map is tied to its spec.  Not offered:
    per-eye maps, a windowed history (as opposed to the decayed one), anisotropic or screen-millimetre sigmas, gradients, EVE.forward
    (its create_images path keeps the torch restatement), maps larger than 2048 per axis.  (Areas of interest and dwell-per-region
    tables: AoiSpec.)"""

    def __init__(self, name='gaze_history', source=None, valid_key=None, size=None, sigma=None, decay_per_ms=None, weight='frame',
                 max_gap_s=0.075, fps=None, floor=0.0, normalize=False, per_frame=False):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        if not isinstance(name, str) or not name:
            raise ValueError('GazeHistorySpec: name must be a non-empty string, got %r' % (name,))
        if source is not None and source not in GAZE_HISTORY_SOURCES:
            raise ValueError('GazeHistorySpec: source must be None or one of %s, got %r' % (', '.join(GAZE_HISTORY_SOURCES), source))
        if valid_key is not None and (not isinstance(valid_key, str) or not valid_key):
            raise ValueError('GazeHistorySpec: valid_key must be None or the key of a [B, Tc] entry, got %r' % (valid_key,))
        if size is not None:
            axis = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 1 <= int(v) <= GAZE_HISTORY_MAX_AXIS
            if not isinstance(size, (tuple, list)) or len(size) != 2 or not axis(size[0]) or not axis(size[1]):
                raise ValueError('GazeHistorySpec: size must be (MW, MH), integers in 1 .. %d, got %r' % (GAZE_HISTORY_MAX_AXIS, size))
            size = (int(size[0]), int(size[1]))
        if sigma is not None and (not number(sigma) or not sigma > 0):
            raise ValueError('GazeHistorySpec: sigma must be a finite number > 0, got %r' % (sigma,))
        if decay_per_ms is not None and (not number(decay_per_ms) or not 0 < decay_per_ms <= 1):
            raise ValueError('GazeHistorySpec: decay_per_ms must lie in (0, 1], got %r' % (decay_per_ms,))
        if weight not in ('frame', 'seconds'):
            raise ValueError("GazeHistorySpec: weight must be 'frame' or 'seconds', got %r" % (weight,))
        if not number(max_gap_s) or not max_gap_s > 0:
            raise ValueError('GazeHistorySpec: max_gap_s must be a finite number > 0, got %r' % (max_gap_s,))
        if fps is not None and (not number(fps) or not fps > 0):
            raise ValueError('GazeHistorySpec: fps must be a finite number > 0, got %r' % (fps,))
        if not number(floor) or floor < 0:
            raise ValueError('GazeHistorySpec: floor must be a finite number >= 0, got %r' % (floor,))
        self.name, self.source, self.valid_key, self.size, self.weight = name, source, valid_key, size, weight
        self.sigma = None if sigma is None else float(sigma)
        self.decay_per_ms = None if decay_per_ms is None else float(decay_per_ms)
        self.max_gap_s, self.fps, self.floor = float(max_gap_s), None if fps is None else float(fps), float(floor)
        self.normalize, self.per_frame = bool(normalize), bool(per_frame)

    def key(self):
        return (self.name, self.source, self.valid_key, self.size, self.sigma, self.decay_per_ms, self.weight, self.max_gap_s, self.fps,
                self.floor, self.normalize, self.per_frame)

    def __eq__(self, other):
        return isinstance(other, GazeHistorySpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'GazeHistorySpec(name=%r, source=%r, valid_key=%r, size=%r, sigma=%r, decay_per_ms=%r, weight=%r, max_gap_s=%r, fps=%r, ' \
               'floor=%r, normalize=%r, per_frame=%r)' % self.key()

    def resolved(self, config=None):
        """-> (size (MW, MH), sigma, decay_per_ms) with the config's values where the spec leaves them open."""
        from .config import get_config
        cfg = config if config is not None else get_config()
        size = self.size if self.size is not None else (int(cfg.gaze_heatmap_size[0]), int(cfg.gaze_heatmap_size[1]))
        sigma = self.sigma if self.sigma is not None else float(cfg.gaze_heatmap_sigma_history)
        decay = self.decay_per_ms if self.decay_per_ms is not None else float(cfg.gaze_history_map_decay_per_ms)
        if not (1 <= size[0] <= GAZE_HISTORY_MAX_AXIS and 1 <= size[1] <= GAZE_HISTORY_MAX_AXIS) or not sigma > 0 or not 0 < decay <= 1:
            raise ValueError('GazeHistorySpec: the config gives size %r, sigma %r, decay_per_ms %r' % (size, sigma, decay))
        return size, sigma, decay

    def launch_params(self, config=None):
        """-> the two launches' scalars, computed here in double: size, alpha = -0.5 / sigma^2, ln_decay = log(decay_per_ms), gain = 1
        or 1 / (2 pi sigma^2), and the spec's own numbers."""
        import math
        size, sigma, decay = self.resolved(config)
        return {'size': size, 'alpha': -0.5 / (sigma * sigma), 'ln_decay': math.log(decay), 'seconds': self.weight == 'seconds',
                'max_gap_s': self.max_gap_s, 'fps': self.fps, 'floor': self.floor,
                'gain': 1.0 / (2.0 * math.pi * sigma * sigma) if self.normalize else 1.0}


def _bool_rows(t, shape, what):
    if not torch.is_tensor(t) or t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != shape:
        raise TypeError('%s must be bool or uint8 %s' % (what, list(shape)))
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def gaze_history(spec, screen_size, pog_px=None, heatmaps=None, frame_time=None, valid=None, lengths=None):
    """The gaze history of S recorded streams, stand-alone and from fresh state: spec a GazeHistorySpec (its source and valid_key are
    not looked at); screen_size (W, H) of the pixels pog_px is in; pog_px float32 [S, T, 2], or heatmaps float32 [S, T, MH, MW] or
    [S, T, 1, MH, MW] (the heat source) -- one of the two; frame_time None (then spec.fps) or float64 [S, T] seconds; valid None or bool /
    uint8 [S, T]; lengths None or int32 [S] on the device.  The two launches of EVEStream.step(history=...).  -> {<name>: float32
    [S, MH, MW], <name>_frames: float32 [S, T, MH, MW] (with per_frame), 'state': float64 [S, 8]} as device tensors; the host does not
    wait.  Not offered: see GazeHistorySpec."""
    if not isinstance(spec, GazeHistorySpec):
        raise ValueError('gaze_history: spec must be an eve_amd.GazeHistorySpec, got %s' % type(spec).__name__)
    if (pog_px is None) == (heatmaps is None):
        raise ValueError('gaze_history: pog_px or heatmaps, one of the two')
    P = spec.launch_params()
    MW, MH = P['size']
    if pog_px is not None:
        if not torch.is_tensor(pog_px) or pog_px.dtype != torch.float32 or pog_px.dim() != 3 or pog_px.shape[2] != 2 or pog_px.numel() == 0:
            raise TypeError('gaze_history: pog_px must be float32 [S, T, 2], got %s %s' % (getattr(pog_px, 'dtype', type(pog_px)),
                                                                                          tuple(getattr(pog_px, 'shape', ()))))
        S, T = pog_px.shape[:2]
        dev, pog_px = pog_px.device, pog_px.contiguous()
    else:
        if (not torch.is_tensor(heatmaps) or heatmaps.dtype != torch.float32 or heatmaps.dim() not in (4, 5) or heatmaps.numel() == 0 or
                tuple(heatmaps.shape[-2:]) != (MH, MW) or (heatmaps.dim() == 5 and heatmaps.shape[2] != 1)):
            raise TypeError('gaze_history: heatmaps must be float32 [S, T, %d, %d] (the spec\'s size), got %s %s' % (
                MH, MW, getattr(heatmaps, 'dtype', type(heatmaps)), tuple(getattr(heatmaps, 'shape', ()))))
        S, T = heatmaps.shape[:2]
        dev, heatmaps = heatmaps.device, heatmaps.reshape(S, T, MH, MW).contiguous()
    if frame_time is None and spec.fps is None:
        raise ValueError('gaze_history: frame_time, or a spec with fps')
    if frame_time is not None and (not torch.is_tensor(frame_time) or frame_time.dtype != torch.float64 or tuple(frame_time.shape) != (S, T)):
        raise TypeError('gaze_history: frame_time must be float64 [%d, %d] seconds' % (S, T))
    if valid is not None:
        valid = _bool_rows(valid, (S, T), 'gaze_history: valid')
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,)):
        raise TypeError('gaze_history: lengths must be an int32 [%d] tensor' % S)
    k = default_kernels()
    state = torch.zeros((S, 8), dtype=torch.float64, device=dev)
    maps = torch.zeros((S, MH, MW), dtype=torch.float32, device=dev)
    coef, clear = k.gaze_history_plan(P, screen_size, state, T, pog=pog_px, frame_time=None if frame_time is None else frame_time.contiguous(),
                                      valid=valid, lengths=None if lengths is None else lengths.contiguous())
    frames = k.gaze_history_update(P, coef, clear, maps, heat=heatmaps, per_frame=spec.per_frame)
    out = {spec.name: maps, 'state': state}
    if spec.per_frame:
        out[spec.name + '_frames'] = frames
    return out


AOI_SOURCES = ('PoG_px_initial', 'PoG_px_final', 'PoG_px_filtered', 'fixation_px')
AOI_MAX = 64                                     # areas of interest per table
AOI_ROW = 36                                     # floats per area: kind, vertex count, two reserved, 32 coordinates
AOI_MAX_VERTICES = 16
AOI_KEYS = ('id', 'mask', 'visit_ms')            # the per-frame results, as <name>_<key>


class AoiSpec(object):
    """What EVEStream.step(chunk, aoi=spec) adds to the step (eve_gaze_aoi): per frame the area of interest the point of gaze is in,
    and per stream the visits, the dwell table and the transition matrix over the chunk's aoi_shapes (data.aoi_shapes builds them).
      name            the prefix of the result keys <name>_id, <name>_mask, <name>_visit_ms, and the name of the tallies
      num_aois        A, 1 .. 64: the rows of the shape table
      source          'PoG_px_initial', 'PoG_px_final', 'PoG_px_filtered', 'fixation_px' (the last two need events= in the same step), or
                      None: PoG_px_final with a RefineNet, else PoG_px_initial (the rule the events use)
      valid_key       None or the key of a bool / uint8 [B, Tc] entry of the result or the chunk, ANDed into the frame's usability
                      (source='fixation_px', valid_key='fixating': the fixation-based AOI analysis)
      fps             for chunks without frame_time (float64 [B, Tc] seconds, which wins when both are there)
      max_gap_s       two samples further apart than this are not connected: the open visit ends at its last sample
      use_fixations   True: count fixations per AOI and per visit from the events stage's fixation_id / fixating (needs events=);
                      False: never; None: where events= runs in the same step
    Instances compare and hash by value: the spec is part of a captured graph's key, and the tallies are tied to their spec.  Not
    offered: label-map AOIs, minimum visit durations or border hysteresis, per-eye AOIs, polygon margins, AOI outlines in the overlay,
    gradients, EVE.forward."""

    def __init__(self, name='aoi', num_aois=None, source=None, valid_key=None, fps=None, max_gap_s=0.075, use_fixations=None):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        if not isinstance(name, str) or not name:
            raise ValueError('AoiSpec: name must be a non-empty string, got %r' % (name,))
        if isinstance(num_aois, bool) or not isinstance(num_aois, (int, np.integer)) or not 1 <= int(num_aois) <= AOI_MAX:
            raise ValueError('AoiSpec: num_aois must be an integer in 1 .. %d, got %r' % (AOI_MAX, num_aois))
        if source is not None and source not in AOI_SOURCES:
            raise ValueError('AoiSpec: source must be None or one of %s, got %r' % (', '.join(AOI_SOURCES), source))
        if valid_key is not None and (not isinstance(valid_key, str) or not valid_key):
            raise ValueError('AoiSpec: valid_key must be None or the key of a [B, Tc] entry, got %r' % (valid_key,))
        if fps is not None and (not number(fps) or not fps > 0):
            raise ValueError('AoiSpec: fps must be a finite number > 0, got %r' % (fps,))
        if not number(max_gap_s) or not max_gap_s > 0:
            raise ValueError('AoiSpec: max_gap_s must be a finite number > 0, got %r' % (max_gap_s,))
        if use_fixations is not None and not isinstance(use_fixations, bool):
            raise ValueError('AoiSpec: use_fixations must be None, True or False, got %r' % (use_fixations,))
        self.name, self.num_aois, self.source, self.valid_key = name, int(num_aois), source, valid_key
        self.fps, self.max_gap_s, self.use_fixations = None if fps is None else float(fps), float(max_gap_s), use_fixations

    def key(self):
        return (self.name, self.num_aois, self.source, self.valid_key, self.fps, self.max_gap_s, self.use_fixations)

    def __eq__(self, other):
        return isinstance(other, AoiSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'AoiSpec(name=%r, num_aois=%r, source=%r, valid_key=%r, fps=%r, max_gap_s=%r, use_fixations=%r)' % self.key()


def aoi_shapes(shapes, num_aois, margin_px=0.0):
    """The shape table of eve_gaze_aoi, float32 [num_aois, 36] (a CPU tensor), from a list of
      ('rect', x0, y0, x1, y1)          x0 <= x < x1 and y0 <= y < y1 (half open, so tiles that share an edge do not overlap)
      ('ellipse', cx, cy, rx, ry)       rx, ry > 0
      ('polygon', [(x, y), ...])        3 .. 16 vertices, even-odd rule
      None                              a disabled row
    in actual_screen_size pixels.  The order is the z-order: a frame's AOI is the first row that contains the point.  Rows past the
    list are disabled.  margin_px >= 0 grows every rectangle and every ellipse's radii by that much on each side (the usual allowance
    for the tracker's error); with a margin a polygon is refused.  A row is [kind (0 disabled, 1 rectangle, 2 ellipse, 3 polygon), n,
    0, 0, coordinates ...].  Stack tables to [B, A, 36], or to [B, Tc, A, 36] for regions that move from frame to frame."""
    number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
    if isinstance(num_aois, bool) or not isinstance(num_aois, (int, np.integer)) or not 1 <= int(num_aois) <= AOI_MAX:
        raise ValueError('aoi_shapes: num_aois must be an integer in 1 .. %d, got %r' % (AOI_MAX, num_aois))
    if not number(margin_px) or margin_px < 0:
        raise ValueError('aoi_shapes: margin_px must be a finite number >= 0, got %r' % (margin_px,))
    shapes = list(shapes)
    if len(shapes) > num_aois:
        raise ValueError('aoi_shapes: %d shapes for num_aois = %d' % (len(shapes), num_aois))
    table = np.zeros((int(num_aois), AOI_ROW), dtype=np.float32)
    m = float(margin_px)
    for i, s in enumerate(shapes):
        if s is None:
            continue
        if not isinstance(s, (tuple, list)) or not s or s[0] not in ('rect', 'ellipse', 'polygon'):
            raise ValueError('aoi_shapes: shape %d must be None or start with \'rect\', \'ellipse\' or \'polygon\', got %r' % (i, s))
        if s[0] == 'polygon':
            if m != 0.0:
                raise ValueError('aoi_shapes: shape %d: a margin on a polygon is not offered' % i)
            pts = list(s[1]) if len(s) == 2 and isinstance(s[1], (tuple, list, np.ndarray)) else None
            if pts is None or not 3 <= len(pts) <= AOI_MAX_VERTICES or \
                    not all(isinstance(p, (tuple, list, np.ndarray)) and len(p) == 2 and number(p[0]) and number(p[1]) for p in pts):
                raise ValueError('aoi_shapes: shape %d: a polygon is (\'polygon\', [(x, y), ...]) with 3 .. %d finite vertices, got %r' % (
                    i, AOI_MAX_VERTICES, s))
            table[i, 0], table[i, 1] = 3, len(pts)
            table[i, 4:4 + 2 * len(pts)] = np.asarray(pts, dtype=np.float64).reshape(-1)
            continue
        if len(s) != 5 or not all(number(v) for v in s[1:]):
            raise ValueError('aoi_shapes: shape %d: (%r, four finite numbers), got %r' % (i, s[0], s))
        c = [float(v) for v in s[1:]]
        if s[0] == 'rect':
            if not (c[0] < c[2] and c[1] < c[3]):
                raise ValueError('aoi_shapes: shape %d: a rectangle needs x0 < x1 and y0 < y1, got %r' % (i, s))
            with np.errstate(over='ignore'):     # (what does not fit float32 is refused below)
                table[i, 0], table[i, 4:8] = 1, (c[0] - m, c[1] - m, c[2] + m, c[3] + m)
        else:
            if not (c[2] > 0 and c[3] > 0):
                raise ValueError('aoi_shapes: shape %d: an ellipse needs rx > 0 and ry > 0, got %r' % (i, s))
            table[i, 0], table[i, 4:8] = 2, (c[0], c[1], c[2] + m, c[3] + m)
    if not np.isfinite(table).all():
        raise ValueError('aoi_shapes: a coordinate does not fit float32')
    return torch.from_numpy(table)


def gaze_aoi(spec, pog_px, shapes, frame_time=None, valid=None, lengths=None, fixation_id=None, fixating=None, visit_capacity=256):
    """The areas of interest of S recorded streams, stand-alone and from fresh state: spec an AoiSpec (its name prefixes the per-frame
    keys; source, valid_key and use_fixations are not looked at); pog_px float32 [S, T, 2] (actual_screen_size pixels); shapes float32
    [S, A, 36] or [S, T, A, 36] (aoi_shapes), A = spec.num_aois; frame_time None (then spec.fps) or float64 [S, T] seconds; valid None or
    bool / uint8 [S, T]; lengths None or int32 [S] on the device; fixation_id int32 [S, T] with fixating bool / uint8 [S, T] (the events'
    outputs), or neither.  One eve_gaze_aoi launch, which also closes the visits still open at the clip's end.  -> <name>_id int32
    [S, T] (the AOI, -1 outside all, -2 not a sample), <name>_mask int64 [S, T] (bit a: AOI a contains the point), <name>_visit_ms float32
    [S, T], plus table float64 [S, A + 1, 8] (rows (dwell_s, samples, visits, t_first_entry, t_last, fixations, t_first_fixation, 0);
    row A: no AOI), transitions int32 [S, A + 1, A] (row A: the first visit), visits float64 [S, visit_capacity, 8] (rows (aoi, t_enter,
    t_last, samples, fixations, visit_index, 0, 0)), visit_count and visit_dropped int32 [S], and state float64 [S, 16]; the host does
    not wait.  Not offered: see AoiSpec."""
    if not isinstance(spec, AoiSpec):
        raise ValueError('gaze_aoi: spec must be an eve_amd.AoiSpec, got %s' % type(spec).__name__)
    if not torch.is_tensor(pog_px) or pog_px.dtype != torch.float32 or pog_px.dim() != 3 or pog_px.shape[2] != 2 or pog_px.numel() == 0:
        raise TypeError('gaze_aoi: pog_px must be float32 [S, T, 2], got %s %s' % (getattr(pog_px, 'dtype', type(pog_px)),
                                                                                 tuple(getattr(pog_px, 'shape', ()))))
    S, T = pog_px.shape[:2]
    A = spec.num_aois
    if not torch.is_tensor(shapes) or shapes.dtype != torch.float32 or tuple(shapes.shape) not in ((S, A, AOI_ROW), (S, T, A, AOI_ROW)):
        raise TypeError('gaze_aoi: shapes must be float32 [%d, %d, 36] or [%d, %d, %d, 36], got %s %s' % (
            S, A, S, T, A, getattr(shapes, 'dtype', type(shapes)), tuple(getattr(shapes, 'shape', ()))))
    if frame_time is None and spec.fps is None:
        raise ValueError('gaze_aoi: frame_time, or a spec with fps')
    if frame_time is not None and (not torch.is_tensor(frame_time) or frame_time.dtype != torch.float64 or tuple(frame_time.shape) != (S, T)):
        raise TypeError('gaze_aoi: frame_time must be float64 [%d, %d] seconds' % (S, T))
    if valid is not None:
        valid = _bool_rows(valid, (S, T), 'gaze_aoi: valid')
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,)):
        raise TypeError('gaze_aoi: lengths must be an int32 [%d] tensor' % S)
    if (fixation_id is None) != (fixating is None):
        raise ValueError('gaze_aoi: fixation_id and fixating come together')
    if fixation_id is not None:
        if not torch.is_tensor(fixation_id) or fixation_id.dtype != torch.int32 or tuple(fixation_id.shape) != (S, T):
            raise TypeError('gaze_aoi: fixation_id must be int32 [%d, %d]' % (S, T))
        fixation_id, fixating = fixation_id.contiguous(), _bool_rows(fixating, (S, T), 'gaze_aoi: fixating')
    if isinstance(visit_capacity, bool) or not isinstance(visit_capacity, (int, np.integer)) or visit_capacity < 1:
        raise ValueError('gaze_aoi: visit_capacity must be an integer >= 1, got %r' % (visit_capacity,))
    visit_capacity = int(visit_capacity)
    dev = pog_px.device
    state, table, trans, visits, count, dropped = aoi_buffers(S, A, visit_capacity, dev)
    out = default_kernels().gaze_aoi(pog_px.contiguous(), shapes.contiguous(), spec, state, table, trans, visits, count, dropped,
                                     frame_time=None if frame_time is None else frame_time.contiguous(), valid=valid,
                                     fixation_id=fixation_id, fixating=fixating, lengths=None if lengths is None else lengths.contiguous(),
                                     flush=torch.ones((S,), dtype=torch.int32, device=dev))
    out = {'%s_%s' % (spec.name, k_): v for k_, v in out.items()}
    out.update(table=table, transitions=trans, visits=visits, visit_count=count, visit_dropped=dropped, state=state)
    return out


def aoi_buffers(S, A, visit_capacity, device):
    """-> (state float64 [S, 16], table float64 [S, A + 1, 8], trans int32 [S, A + 1, A], visits float64 [S, visit_capacity, 8], count and
    dropped int32 [S]) of S streams that have seen nothing: what eve_gaze_aoi carries."""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)
    return (z((S, 16), torch.float64), z((S, A + 1, 8), torch.float64), z((S, A + 1, A), torch.int32), z((S, visit_capacity, 8), torch.float64),
            z((S,), torch.int32), z((S,), torch.int32))


PUPIL_KEYS = ('mm', 'raw_mm', 'velocity', 'change_mm', 'change_pct', 'valid', 'eye_used', 'eye_reason', 'event')      # as <name>_<key>
PUPIL_STATE = 32                                 # doubles per stream of eve_pupil_track's state row
PUPIL_TABLE = 24                                 # ... and of its table


class PupilSpec(object):
    """What EVEStream.step(chunk, pupil=spec) adds to the step (eve_pupil_track): EyeNet's two pupil sizes become one validated,
    binocularly fused, low-passed, light- and baseline-corrected trace per stream, with a table of tallies and a store of dilation /
    constriction episodes.
      name              the prefix of the result keys <name>_mm, _raw_mm, _velocity, _change_mm, _change_pct, _valid, _eye_used,
                        _eye_reason, _event, and the name of the tallies
      fps               for chunks without frame_time (float64 [B, Tc] seconds, which wins when both are there)
      min_mm, max_mm    the accepted range of a size (1.5 .. 9 mm: the range filter of Kret & Sjak-Shie 2019, "Preprocessing pupil
                        size data", Behav. Res. Methods 51)
      max_speed_mm_s    an eye whose size moves faster than this against its last accepted one is rejected -- their dilation-speed
                        criterion with a fixed bound in place of the non-causal MAD (10 mm/s: above the 5 .. 7 mm/s peak constriction
                        velocity of the light reflex, Bremner 2012, "Pupillometric evaluation of the dynamics of the pupillary
                        response to a brief light stimulus", IOVS 53)
      max_gap_s         samples further apart than this are not connected (the filter restarts, an episode ends), and a rejected eye
                        is re-admitted untested after it (0.25 s: the longest gap Kret & Sjak-Shie bridge)
      offset_rate       in (0, 1]: how fast the running left - right offset follows, per binocular sample (0.05)
      cutoff_hz         the one-pole low pass of the fused size (4 Hz: Jackson & Sirois 2009, Kret & Sjak-Shie 2019)
      light_tau_s       the time constant of the luminance's own low pass, standing for the lag of the light reflex (0.5 s: Ellis
                        1981, "The pupillary light reflex in normal subjects", Br. J. Ophthalmol. 65)
      baseline_tau_s    None: no follower; else the time constant of the slow baseline used where the chunk has no pupil_baseline marks
      dilate_mm_s, constrict_mm_s    the velocity above / below which a sample dilates / constricts (0.15 and 0.3 mm/s)
      min_amplitude_mm  episodes that move the filtered size by less are not stored (0.1 mm: the lower end of task-evoked responses,
                        Beatty 1982, "Task-evoked pupillary responses", Psychol. Bull. 91)
    Instances compare and hash by value: the spec is part of a captured graph's key, and the tallies are tied to their spec.  The
    light covariate comes with the chunk as pupil_luminance, or from luminance=ScreenLuminanceSpec(...) in the same step.  Not
    offered: non-causal blink padding and interpolation across gaps, foreshortening correction, per-eye filtered traces, wavelet indices (IPA / LHIPA),
    per-fixation or per-AOI pupil means, gradients, EVE.forward, the overlay."""

    def __init__(self, name='pupil', fps=None, min_mm=1.5, max_mm=9.0, max_speed_mm_s=10.0, max_gap_s=0.25, offset_rate=0.05, cutoff_hz=4.0,
                 light_tau_s=0.5, baseline_tau_s=None, dilate_mm_s=0.15, constrict_mm_s=0.3, min_amplitude_mm=0.1):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        if not isinstance(name, str) or not name:
            raise ValueError('PupilSpec: name must be a non-empty string, got %r' % (name,))
        if fps is not None and (not number(fps) or not fps > 0):
            raise ValueError('PupilSpec: fps must be a finite number > 0, got %r' % (fps,))
        for field, v in (('min_mm', min_mm), ('max_mm', max_mm), ('max_speed_mm_s', max_speed_mm_s), ('max_gap_s', max_gap_s),
                         ('cutoff_hz', cutoff_hz), ('light_tau_s', light_tau_s), ('dilate_mm_s', dilate_mm_s), ('constrict_mm_s', constrict_mm_s)):
            if not number(v) or not v > 0:
                raise ValueError('PupilSpec: %s must be a finite number > 0, got %r' % (field, v))
        if not min_mm < max_mm:
            raise ValueError('PupilSpec: min_mm must be below max_mm, got %r and %r' % (min_mm, max_mm))
        if not number(offset_rate) or not 0 < offset_rate <= 1:
            raise ValueError('PupilSpec: offset_rate must lie in (0, 1], got %r' % (offset_rate,))
        if baseline_tau_s is not None and (not number(baseline_tau_s) or not baseline_tau_s > 0):
            raise ValueError('PupilSpec: baseline_tau_s must be None or a finite number > 0, got %r' % (baseline_tau_s,))
        if not number(min_amplitude_mm) or not min_amplitude_mm >= 0:
            raise ValueError('PupilSpec: min_amplitude_mm must be a finite number >= 0, got %r' % (min_amplitude_mm,))
        self.name, self.fps = name, None if fps is None else float(fps)
        self.min_mm, self.max_mm, self.max_speed_mm_s, self.max_gap_s = float(min_mm), float(max_mm), float(max_speed_mm_s), float(max_gap_s)
        self.offset_rate, self.cutoff_hz, self.light_tau_s = float(offset_rate), float(cutoff_hz), float(light_tau_s)
        self.baseline_tau_s = None if baseline_tau_s is None else float(baseline_tau_s)
        self.dilate_mm_s, self.constrict_mm_s, self.min_amplitude_mm = float(dilate_mm_s), float(constrict_mm_s), float(min_amplitude_mm)

    def key(self):
        return (self.name, self.fps, self.min_mm, self.max_mm, self.max_speed_mm_s, self.max_gap_s, self.offset_rate, self.cutoff_hz,
                self.light_tau_s, self.baseline_tau_s, self.dilate_mm_s, self.constrict_mm_s, self.min_amplitude_mm)

    def __eq__(self, other):
        return isinstance(other, PupilSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return ('PupilSpec(name=%r, fps=%r, min_mm=%r, max_mm=%r, max_speed_mm_s=%r, max_gap_s=%r, offset_rate=%r, cutoff_hz=%r, light_tau_s=%r, '
                'baseline_tau_s=%r, dilate_mm_s=%r, constrict_mm_s=%r, min_amplitude_mm=%r)') % self.key()


def pupil_buffers(S, capacity, device):
    """-> (state float64 [S, 32], table float64 [S, 24], light float64 [S, 4], store float64 [S, capacity, 8], count and dropped int32
    [S]) of S streams that have seen nothing: what eve_pupil_track carries (include/eve_hip.h has the rows)."""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)
    return (z((S, PUPIL_STATE), torch.float64), z((S, PUPIL_TABLE), torch.float64), z((S, 4), torch.float64), z((S, capacity, 8), torch.float64),
            z((S,), torch.int32), z((S,), torch.int32))


def pupil_track(spec, left, right, eye_valid=None, frame_time=None, lengths=None, luminance=None, baseline_mark=None, light=None,
                episode_capacity=256):
    """The pupillometry of S recorded streams, stand-alone and from fresh state: spec a PupilSpec (its name prefixes the per-frame
    keys); left, right float32 [S, T] pupil sizes in mm (EyeNet's <side>_pupil_size); eye_valid None or bool / uint8 [S, T, 2];
    frame_time None (then spec.fps) or float64 [S, T] seconds; lengths None or int32 [S] on the device; luminance None or float32
    [S, T]; baseline_mark None or bool / uint8 [S, T]; light None or float64 [S, 4] rows (has_gain, gain, ref, 0).  One eve_pupil_track
    launch, which also closes the episodes still open at the clip's end.  -> <name>_mm, _raw_mm, _velocity, _change_mm, _change_pct
    float32 [S, T] (NaN where the frame is no sample), <name>_valid uint8 [S, T], <name>_eye_used and _eye_reason uint8 [S, T, 2] (bit 1
    withheld, 2 not finite, 4 range, 8 speed), <name>_event uint8 [S, T] (1 dilating, 2 constricting), plus table float64 [S, 24],
    episodes float64 [S, episode_capacity, 8] (rows (phase, t_start, t_end, d_start, d_end, peak |velocity|, samples, Lf at the start)),
    episode_count and episode_dropped int32 [S], light and state float64 [S, 4] and [S, 32]; the host does not wait.  Not offered: see
    PupilSpec."""
    if not isinstance(spec, PupilSpec):
        raise ValueError('pupil_track: spec must be an eve_amd.PupilSpec, got %s' % type(spec).__name__)
    for name, t in (('left', left), ('right', right)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.numel() == 0:
            raise TypeError('pupil_track: %s must be float32 [S, T], got %s %s' % (name, getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
    S, T = left.shape
    if tuple(right.shape) != (S, T):
        raise TypeError('pupil_track: right must be float32 [%d, %d] like left, got %s' % (S, T, tuple(right.shape)))
    if frame_time is None and spec.fps is None:
        raise ValueError('pupil_track: frame_time, or a spec with fps')
    if frame_time is not None and (not torch.is_tensor(frame_time) or frame_time.dtype != torch.float64 or tuple(frame_time.shape) != (S, T)):
        raise TypeError('pupil_track: frame_time must be float64 [%d, %d] seconds' % (S, T))
    if eye_valid is not None:
        eye_valid = _bool_rows(eye_valid, (S, T, 2), 'pupil_track: eye_valid')
    if baseline_mark is not None:
        baseline_mark = _bool_rows(baseline_mark, (S, T), 'pupil_track: baseline_mark')
    if luminance is not None and (not torch.is_tensor(luminance) or luminance.dtype != torch.float32 or tuple(luminance.shape) != (S, T)):
        raise TypeError('pupil_track: luminance must be float32 [%d, %d]' % (S, T))
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,)):
        raise TypeError('pupil_track: lengths must be an int32 [%d] tensor' % S)
    if isinstance(episode_capacity, bool) or not isinstance(episode_capacity, (int, np.integer)) or episode_capacity < 1:
        raise ValueError('pupil_track: episode_capacity must be an integer >= 1, got %r' % (episode_capacity,))
    dev = left.device
    state, table, light_, store, count, dropped = pupil_buffers(S, int(episode_capacity), dev)
    if light is not None:
        if not torch.is_tensor(light) or light.dtype != torch.float64 or tuple(light.shape) != (S, 4):
            raise TypeError('pupil_track: light must be float64 [%d, 4] rows (has_gain, gain, ref, 0)' % S)
        light_.copy_(light)
    out = default_kernels().pupil_track(torch.stack([left, right]), spec, state, table, light_, store, count, dropped, eye_valid=eye_valid,
                                        frame_time=None if frame_time is None else frame_time.contiguous(),
                                        lengths=None if lengths is None else lengths.contiguous(),
                                        luminance=None if luminance is None else luminance.contiguous(), baseline_mark=baseline_mark,
                                        flush=torch.ones((S,), dtype=torch.int32, device=dev))
    out = {'%s_%s' % (spec.name, k_): v for k_, v in out.items()}
    out.update(table=table, episodes=store, episode_count=count, episode_dropped=dropped, light=light_, state=state)
    return out


# ------------------------------------------------------------------------------------------------ screen luminance
LUMINANCE_SOURCES = AOI_SOURCES                  # the points a disc can follow
LUMINANCE_WEIGHTS = {'rec709': (13933, 46871, 4732)}      # (kr, kg, kb) in 1 / 65536, summing to 65536
LUMINANCE_MAX_DISCS = 4                          # what eve_screen_luminance takes
LUMINANCE_MAX_RADIUS = 16384                     # ... in capture pixels


def display_response(kind='srgb', gamma=None, measured=None):
    """The display's linearisation as eve_screen_luminance reads it: a uint16 [3, 256] CPU tensor, entry [c][v] the relative light
    of channel c at the 8-bit value v, scaled to 65535 -- floor(65535 * f(v / 255) + 0.5) in float64.
      kind='srgb'      sRGB's EOTF: c / 12.92 up to 0.04045, then ((c + 0.055) / 1.055) ** 2.4
      kind='gamma'     the power law (v / 255) ** gamma, gamma a finite number > 0
      kind='measured'  measured: a [256] curve for all three channels or a [3, 256] one per channel, values in 0 .. 1
    Anything else raises ValueError."""
    v = np.arange(256, dtype=np.float64) / 255.0
    if kind == 'srgb':
        if gamma is not None or measured is not None:
            raise ValueError("display_response: kind 'srgb' takes neither gamma nor measured")
        f = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    elif kind == 'gamma':
        if measured is not None or isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) or \
                not np.isfinite(gamma) or not gamma > 0:
            raise ValueError("display_response: kind 'gamma' takes gamma, a finite number > 0, and no measured curve, got %r" % (gamma,))
        f = v ** float(gamma)
    elif kind == 'measured':
        f = None if measured is None or gamma is not None else np.asarray(measured, dtype=np.float64)
        if f is None or f.shape not in ((256,), (3, 256)) or not np.isfinite(f).all() or f.min() < 0.0 or f.max() > 1.0:
            raise ValueError("display_response: kind 'measured' takes measured, a [256] or [3, 256] curve of values in 0 .. 1, and no gamma")
    else:
        raise ValueError("display_response: kind must be 'srgb', 'gamma' or 'measured', got %r" % (kind,))
    table = np.floor(65535.0 * np.broadcast_to(f, (3, 256)) + 0.5).astype(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(table))


class ScreenLuminanceSpec(object):
    """What EVEStream.step(chunk, luminance=spec) adds to the step (eve_screen_luminance): per frame the mean relative luminance of the
    screen capture -- every pixel read where it lies, converted, linearised through the display's response, weighted -- over the
    whole screen and over discs around the point of gaze; the light covariate of the pupil trace.
      name        the result keys: <name> float32 [B, Tc] (the whole screen), <name>_gaze [B, Tc, R] (the discs), <name>_covariate
      radii_px    up to four strictly increasing disc radii in actual_screen_size pixels (as aoi_shapes); a radius goes to capture
                  pixels as max(1, round(r * sx))
      source      the point the discs follow: 'PoG_px_initial', 'PoG_px_final', 'PoG_px_filtered', 'fixation_px' (the last two need
                  events= in the same step), or None: PoG_px_final with a RefineNet, else PoG_px_initial
      valid_key   None or the key of a bool / uint8 [B, Tc] entry of the result or the chunk, ANDed into the discs' validity
      response    'srgb', ('gamma', g), or a uint16 [3, 256] table (display_response)
      weights     'rec709', or three integers >= 0 that sum to 65536
      to_pupil    None, or up to 1 + R weights over the columns (whole screen, then the discs): <name>_covariate = sum of w_k * mean_k,
                  a left-to-right chain of float32 products and sums that skips columns of weight 0 (so a disc off the screen, whose
                  mean is NaN, poisons nothing it has no weight in); with pupil= in the same step it is that stage's luminance
    Instances compare and hash by value: the spec is part of a captured graph's key.  The mean of a frame that is not delivered, and
    of a disc without a valid centre or off the screen, is NaN.  Not offered: continuous (eccentricity-weighted) kernels beyond
    concentric discs, per-AOI luminance, 10-bit arithmetic, ambient light, the camera image's luminance, the overlay, gradients,
    EVE.forward."""

    def __init__(self, name='screen_luminance', radii_px=(), source=None, valid_key=None, response='srgb', weights='rec709', to_pupil=(1.0,)):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        if not isinstance(name, str) or not name:
            raise ValueError('ScreenLuminanceSpec: name must be a non-empty string, got %r' % (name,))
        try:
            radii = tuple(radii_px)
        except TypeError:
            radii = None
        if radii is None or len(radii) > LUMINANCE_MAX_DISCS or not all(number(r) and r > 0 for r in radii) or \
                any(b <= a for a, b in zip(radii, radii[1:])):
            raise ValueError('ScreenLuminanceSpec: radii_px must be up to %d strictly increasing finite numbers > 0, got %r' % (
                LUMINANCE_MAX_DISCS, radii_px))
        if source is not None and source not in LUMINANCE_SOURCES:
            raise ValueError('ScreenLuminanceSpec: source must be None or one of %s, got %r' % (', '.join(LUMINANCE_SOURCES), source))
        if valid_key is not None and (not isinstance(valid_key, str) or not valid_key):
            raise ValueError('ScreenLuminanceSpec: valid_key must be None or the key of a [B, Tc] entry, got %r' % (valid_key,))
        if isinstance(response, str):
            if response != 'srgb':
                raise ValueError("ScreenLuminanceSpec: response must be 'srgb', ('gamma', g) or a uint16 [3, 256] table, got %r" % (response,))
            table, response_key = display_response('srgb').numpy(), 'srgb'
        elif isinstance(response, tuple) and len(response) == 2 and response[0] == 'gamma':
            table = display_response('gamma', gamma=response[1]).numpy()
            response_key = ('gamma', float(response[1]))
        else:
            table = response.cpu().numpy() if torch.is_tensor(response) else np.asarray(response)
            if table.dtype != np.uint16 or table.shape != (3, 256):
                raise ValueError("ScreenLuminanceSpec: response must be 'srgb', ('gamma', g) or a uint16 [3, 256] table, got %s %s" % (
                    table.dtype, table.shape))
            table = np.ascontiguousarray(table)
            response_key = ('table', table.tobytes())
        if isinstance(weights, str):
            if weights not in LUMINANCE_WEIGHTS:
                raise ValueError('ScreenLuminanceSpec: weights must be one of %s or three integers, got %r' % (', '.join(LUMINANCE_WEIGHTS), weights))
            weights = LUMINANCE_WEIGHTS[weights]
        try:
            weights = tuple(weights)
        except TypeError:
            weights = ()
        if len(weights) != 3 or not all(isinstance(w, (int, np.integer)) and not isinstance(w, bool) and w >= 0 for w in weights) or \
                sum(int(w) for w in weights) != 65536:
            raise ValueError("ScreenLuminanceSpec: weights must be 'rec709' or three integers >= 0 that sum to 65536, got %r" % (weights,))
        if to_pupil is not None:
            try:
                to_pupil = tuple(to_pupil)
            except TypeError:
                raise ValueError('ScreenLuminanceSpec: to_pupil must be None or a sequence of weights, got %r' % (to_pupil,))
            if len(to_pupil) > 1 + len(radii):
                raise ValueError('ScreenLuminanceSpec: to_pupil holds %d weights for %d columns (the whole screen and %d discs)' % (
                    len(to_pupil), 1 + len(radii), len(radii)))
            if not to_pupil or not all(number(w) for w in to_pupil) or not any(w != 0 for w in to_pupil):
                raise ValueError('ScreenLuminanceSpec: to_pupil must be None or finite weights, one of them not 0, got %r' % (to_pupil,))
            to_pupil = tuple(float(w) for w in to_pupil)
        self.name, self.radii_px, self.source, self.valid_key = name, tuple(float(r) for r in radii), source, valid_key
        self.response, self.weights, self.to_pupil = response_key, tuple(int(w) for w in weights), to_pupil
        self._table = table

    def key(self):
        return (self.name, self.radii_px, self.source, self.valid_key, self.response, self.weights, self.to_pupil)

    def __eq__(self, other):
        return isinstance(other, ScreenLuminanceSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        shown = self.response if self.response == 'srgb' or self.response[0] == 'gamma' else '<a [3, 256] table>'
        return 'ScreenLuminanceSpec(name=%r, radii_px=%r, source=%r, valid_key=%r, response=%r, weights=%r, to_pupil=%r)' % (
            self.name, self.radii_px, self.source, self.valid_key, shown, self.weights, self.to_pupil)

    def response_table(self):
        """-> the uint16 [3, 256] table as a CPU tensor (a copy)."""
        return torch.from_numpy(self._table.copy())

    def result_keys(self):
        """-> the keys the stage adds to a step's result."""
        return (self.name,) + ((self.name + '_gaze',) if self.radii_px else ()) + ((self.name + '_covariate',) if self.to_pupil is not None else ())

    def capture_radii(self, sx, where='screen_luminance'):
        """radii_px in capture pixels, max(1, round(r * sx)) -> a tuple of ints; ValueError where two radii fall together or one
        exceeds what the library takes."""
        radii = tuple(max(1, int(round(r * sx))) for r in self.radii_px)
        if any(b <= a for a, b in zip(radii, radii[1:])) or any(r > LUMINANCE_MAX_RADIUS for r in radii):
            raise ValueError('%s: radii_px %r are %r capture pixels at this capture\'s scale (%g): they must stay strictly increasing and <= %d' % (
                where, self.radii_px, radii, sx, LUMINANCE_MAX_RADIUS))
        return radii


def capture_layout(frames, format, lead, name='frames'):
    """The tight SurfaceLayout of byte-linear frames of one pixel format ('rgb', 'bgr' -- with four channels 'rgba', 'bgra' --, 'nv12',
    'i420', 'yuyv'; kernels.pixel_format_shape has the shapes) with `lead` leading dimensions.  TypeError / ValueError as there."""
    from .kernels import pixel_format_shape
    IH, IW, C = pixel_format_shape(frames, format, lead=lead, name=name)
    return SurfaceLayout(format + 'a' if C == 4 else format, IW, IH)


def luminance_results(spec, mean, B, T):
    """eve_screen_luminance's mean float32 [B * T, 1 + R] -> the stage's results under spec.result_keys()."""
    R = len(spec.radii_px)
    out = {spec.name: mean[:, 0].reshape(B, T)}
    if R:
        out[spec.name + '_gaze'] = mean[:, 1:].reshape(B, T, R)
    if spec.to_pupil is not None:
        cov = None
        for k_, w in enumerate(spec.to_pupil):
            if w == 0:
                continue
            term = mean[:, k_] * w
            cov = term if cov is None else cov + term
        out[spec.name + '_covariate'] = cov.reshape(B, T)
    return out


def screen_luminance(frames, layout_or_format, spec, screen_size, pog_px=None, valid=None, lengths=None, matrix='bt601'):
    """The screen luminance of S recorded streams, stand-alone: frames uint8 [S, T, ...], the captures byte-linear in the pixel format
    layout_or_format names ('rgb', 'bgr', 'nv12', 'i420', 'yuyv') or as surfaces under a SurfaceLayout; spec a ScreenLuminanceSpec
    (source and valid_key are not looked at); screen_size (W, H) of the pixels pog_px and spec.radii_px are in; pog_px float32 [S, T, 2],
    needed iff the spec has radii; valid None or bool / uint8 [S, T] (the discs' validity); lengths None or int32 [S] on the device;
    matrix for the YUV formats.  One eve_screen_luminance launch.  -> the spec's result keys (<name> float32 [S, T], <name>_gaze
    [S, T, R], <name>_covariate [S, T]) plus sums int64 and counts int32 [S, T, 1 + R]; the host does not wait."""
    where = 'screen_luminance'
    if not isinstance(spec, ScreenLuminanceSpec):
        raise ValueError('%s: spec must be an eve_amd.ScreenLuminanceSpec, got %s' % (where, type(spec).__name__))
    W, H = check_screen_size(screen_size, where)
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() < 3:
        raise TypeError('%s: frames must be uint8 [S, T, one frame], got %s %s' % (where, getattr(frames, 'dtype', type(frames)),
                                                                                   tuple(getattr(frames, 'shape', ()))))
    if isinstance(layout_or_format, SurfaceLayout):
        layout = layout_or_format
        surface_frames(frames, layout, 2, name=where + ': frames')
    else:
        layout = capture_layout(frames, layout_or_format, 2, name=where + ': frames')
    S, T = int(frames.shape[0]), int(frames.shape[1])
    R = len(spec.radii_px)
    sx, sy = layout.width / W, layout.height / H
    radii = spec.capture_radii(sx, where)
    if (pog_px is None) != (R == 0):
        raise ValueError('%s: pog_px comes with a spec that has radii_px, and only then' % where)
    if pog_px is not None and (not torch.is_tensor(pog_px) or pog_px.dtype != torch.float32 or tuple(pog_px.shape) != (S, T, 2)):
        raise TypeError('%s: pog_px must be float32 [%d, %d, 2]' % (where, S, T))
    if valid is not None:
        valid = _bool_rows(valid, (S, T), where + ': valid').reshape(S * T)
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,)):
        raise TypeError('%s: lengths must be an int32 [%d] tensor' % (where, S))
    if not frames.is_contiguous():
        raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
    sums, counts, mean = default_kernels().screen_luminance(
        frames.reshape(S * T, -1), layout, spec.response_table().to(frames.device), spec.weights, S, T, radii=radii,
        centres=None if pog_px is None else pog_px.reshape(S * T, 2).contiguous(), sx=sx, sy=sy, centre_valid=valid,
        lengths=None if lengths is None else lengths.contiguous(), matrix=matrix)
    out = luminance_results(spec, mean, S, T)
    out.update(sums=sums.reshape(S, T, 1 + R), counts=counts.reshape(S, T, 1 + R))
    return out


EYE_GATE_KEYS = ('eye_gate_reason', 'eye_openness', 'blink')
EYE_CONTOURS_KEY = 'eye_contours'


def _gate_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and not np.isnan(v)


class BlinkSpec(object):
    """The blink detector of an EyeGateSpec, on the eyelid aspect ratio (the mean of the two lid openings over the eye's width, from
    six eyelid points per eye: the chunk's eye_contours) relative to a baseline that follows the open eye.
      close_ratio        the eye closes when aspect ratio / baseline falls below this
      open_ratio         ... and reopens when it rises above this (> close_ratio: a hysteresis)
      baseline_rate      how fast the baseline follows a falling open-eye ratio, per frame (0 .. 1)
      baseline_rise      how fast it follows a rising one (0 .. 1): a peak follower, so that a first frame taken in the middle of a
                         blink does not keep the baseline down
      hold_frames        frames withheld after a blink, from the reopening frame on (the lid is still moving)
      max_closed_frames  a closure longer than this is a wrong baseline, not a blink: the baseline starts over, nothing is stored
    The defaults are conventional -- closing near two thirds of the open ratio, reopening at three quarters, two frames of
    hold-off, three seconds at 30 frames per second; no recording was available to tune them on.  Compares and hashes by value."""

    def __init__(self, close_ratio=0.65, open_ratio=0.75, baseline_rate=0.02, baseline_rise=0.5, hold_frames=2, max_closed_frames=90):
        for name, v in (('close_ratio', close_ratio), ('open_ratio', open_ratio)):
            if not _gate_number(v) or not 0 < v < np.inf:
                raise ValueError('BlinkSpec: %s must be a finite number > 0, got %r' % (name, v))
        if not open_ratio > close_ratio:
            raise ValueError('BlinkSpec: open_ratio must be above close_ratio, got %r and %r' % (open_ratio, close_ratio))
        for name, v in (('baseline_rate', baseline_rate), ('baseline_rise', baseline_rise)):
            if not _gate_number(v) or not 0 <= v <= 1:
                raise ValueError('BlinkSpec: %s must be a number in 0 .. 1, got %r' % (name, v))
        for name, v, least in (('hold_frames', hold_frames, 0), ('max_closed_frames', max_closed_frames, 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not least <= v <= 1 << 20:
                raise ValueError('BlinkSpec: %s must be an integer in %d .. %d, got %r' % (name, least, 1 << 20, v))
        self.close_ratio, self.open_ratio = float(close_ratio), float(open_ratio)
        self.baseline_rate, self.baseline_rise = float(baseline_rate), float(baseline_rise)
        self.hold_frames, self.max_closed_frames = int(hold_frames), int(max_closed_frames)

    def key(self):
        return (self.close_ratio, self.open_ratio, self.baseline_rate, self.baseline_rise, self.hold_frames, self.max_closed_frames)

    def __eq__(self, other):
        return isinstance(other, BlinkSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'BlinkSpec(close_ratio=%r, open_ratio=%r, baseline_rate=%r, baseline_rise=%r, hold_frames=%r, max_closed_frames=%r)' % self.key()


class EyeGateSpec(object):
    """What EVEStream.step(chunk, gate=spec) decides on the device, per frame and eye, before the masked step consumes it
    (eve_eye_gate): an eye is usable iff no criterion vetoes it.  pose_valid is always a criterion where a pose form is in the
    chunk; every other one is off (None) by default:
      max_reproj_px    the face-landmark solve's face_reproj_rms must not exceed this many pixels
      min_inliers      ... and its face_inliers must reach this count (needs face_huber_px or face_landmarks_raw)
      min_coverage     the share (0 .. 1] of an 8 x 8 lattice over the eye patch that must fall inside the camera frame; with
                       camera_lens the test is made in the undistorted coordinates the warp refers to (an approximation at the edge)
      head_pitch       (lo, hi) radians for <side>_h[..., 0], the head's pitch in the eye's normalised space; an open side: +-inf
      head_yaw_left, head_yaw_right   (lo, hi) for <side>_h[..., 1], PER EYE, so the far eye of a turned head can be dropped before the
                       near one; the signs are eve_eye_pose_normalize's (data.normalize_eyes)
      blink            None or a BlinkSpec: eyelid closure from the chunk's eye_contours, with state carried across steps
    Instances compare and hash by value: the spec is part of a captured graph's key.  Not offered: thresholds learnt per person, a
    closure announced before its first closed frame, blink times in seconds, a mid-chunk reset of stale recurrent state after a long
    gap, coverage through the lens model, gradients, EVE.forward."""

    def __init__(self, max_reproj_px=None, min_inliers=None, min_coverage=None, head_pitch=None, head_yaw_left=None, head_yaw_right=None,
                 blink=None):
        if max_reproj_px is not None and (not _gate_number(max_reproj_px) or not 0 < max_reproj_px < np.inf):
            raise ValueError('EyeGateSpec: max_reproj_px must be None or a finite number > 0, got %r' % (max_reproj_px,))
        if min_inliers is not None and (isinstance(min_inliers, bool) or not isinstance(min_inliers, (int, np.integer)) or
                                        not 1 <= min_inliers <= 255):
            raise ValueError('EyeGateSpec: min_inliers must be None or an integer in 1 .. 255, got %r' % (min_inliers,))
        if min_coverage is not None and (not _gate_number(min_coverage) or not 0 < min_coverage <= 1):
            raise ValueError('EyeGateSpec: min_coverage must be None or a number in (0, 1], got %r' % (min_coverage,))
        ranges = []
        for name, r in (('head_pitch', head_pitch), ('head_yaw_left', head_yaw_left), ('head_yaw_right', head_yaw_right)):
            if r is not None:
                if (not isinstance(r, (tuple, list)) or len(r) != 2 or not all(_gate_number(v) for v in r) or not r[0] <= r[1]):
                    raise ValueError('EyeGateSpec: %s must be None or (lo, hi) radians with lo <= hi, got %r' % (name, r))
                r = (float(r[0]), float(r[1]))
            ranges.append(r)
        if blink is not None and not isinstance(blink, BlinkSpec):
            raise ValueError('EyeGateSpec: blink must be None or an eve_amd.BlinkSpec, got %s' % type(blink).__name__)
        self.max_reproj_px = None if max_reproj_px is None else float(max_reproj_px)
        self.min_inliers = None if min_inliers is None else int(min_inliers)
        self.min_coverage = None if min_coverage is None else float(min_coverage)
        self.head_pitch, self.head_yaw_left, self.head_yaw_right = ranges
        self.blink = blink

    @property
    def min_inside(self):
        """The lattice points (1 .. 64) that min_coverage asks for: ceil(min_coverage * 64)."""
        return None if self.min_coverage is None else min(max(int(np.ceil(self.min_coverage * 64.0)), 1), 64)

    @property
    def head_angles(self):
        return self.head_pitch is not None or self.head_yaw_left is not None or self.head_yaw_right is not None

    def key(self):
        return (self.max_reproj_px, self.min_inliers, self.min_coverage, self.head_pitch, self.head_yaw_left, self.head_yaw_right,
                None if self.blink is None else self.blink.key())

    def __eq__(self, other):
        return isinstance(other, EyeGateSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'EyeGateSpec(max_reproj_px=%r, min_inliers=%r, min_coverage=%r, head_pitch=%r, head_yaw_left=%r, head_yaw_right=%r, ' \
               'blink=%r)' % (self.max_reproj_px, self.min_inliers, self.min_coverage, self.head_pitch, self.head_yaw_left,
                              self.head_yaw_right, self.blink)


def check_eye_contours(contours, B, T, device, where):
    """The chunk's eye_contours: float32 [B, T, 2, 6, 2 | 3] on `device` (ValueError otherwise)."""
    if (not torch.is_tensor(contours) or contours.dtype != torch.float32 or contours.dim() != 5 or
            tuple(contours.shape[:4]) != (B, T, 2, 6) or contours.shape[4] not in (2, 3) or contours.device != device):
        raise ValueError('%s: %s must be a float32 [%d, %d, 2, 6, 2 | 3] tensor on %s (the six eyelid points p1 .. p6 of the left and the '
                         'right eye), got %s %s' % (where, EYE_CONTOURS_KEY, B, T, device, getattr(contours, 'dtype', type(contours)),
                                                   tuple(getattr(contours, 'shape', ()))))


def eye_gate(spec, num_streams, num_frames, pose_valid=None, reproj_rms=None, inliers=None, warps=None, h=None, eye_contours=None,
             frame_size=None, patch_size=None, lengths=None, blink_capacity=256, device=None):
    """The eye gate of S recorded streams x T frames, stand-alone and from fresh state: one eve_eye_gate launch.  spec an
    EyeGateSpec; pose_valid bool / uint8 [S, T, 2]; reproj_rms float32 [S, T]; inliers uint8 [S, T]; warps float32 [2, S, T, 3, 3] (left,
    right; inv(W)) with frame_size (IW, IH) and patch_size (OW, OH); h float32 [2, S, T, 2]; eye_contours float32 [S, T, 2, 6, 2 | 3];
    lengths int32 [S]: device tensors, each None where it is not known.  A criterion of the spec whose input is missing is a
    ValueError.  -> usable, eye_gate_reason, blink (uint8 [S, T, 2]), eye_openness (float32 [S, T, 2]), blinks (float64
    [S, blink_capacity, 4], rows (eye, first tick, last tick, minimum openness)), blink_count, blink_dropped (int32 [S]) and
    gate_state (float64 [S, 2, 8]); the host does not wait."""
    if not isinstance(spec, EyeGateSpec):
        raise ValueError('eye_gate: spec must be an eve_amd.EyeGateSpec, got %s' % type(spec).__name__)
    S, T = int(num_streams), int(num_frames)
    for name, on, t in (('max_reproj_px', spec.max_reproj_px is not None, reproj_rms), ('min_inliers', spec.min_inliers is not None, inliers),
                        ('min_coverage', spec.min_coverage is not None, warps), ('head_pitch / head_yaw', spec.head_angles, h),
                        ('blink', spec.blink is not None, eye_contours)):
        if on and t is None:
            raise ValueError('eye_gate: the spec\'s %s has no input to test' % name)
    if spec.min_coverage is not None and (frame_size is None or patch_size is None):
        raise ValueError('eye_gate: min_coverage needs frame_size (IW, IH) and patch_size (OW, OH)')
    if isinstance(blink_capacity, bool) or not isinstance(blink_capacity, int) or blink_capacity < 1:
        raise ValueError('eye_gate: blink_capacity must be an integer >= 1, got %r' % (blink_capacity,))
    tensors = [t for t in (pose_valid, reproj_rms, inliers, warps, h, eye_contours, lengths) if t is not None]
    dev = tensors[0].device if tensors else torch.device(device if device is not None else 'cuda')
    if pose_valid is not None:
        pose_valid = pose_valid.contiguous()
        pose_valid = pose_valid.view(torch.uint8) if pose_valid.dtype == torch.bool else pose_valid
    state = torch.zeros((S, 2, 8), dtype=torch.float64, device=dev)
    store = torch.zeros((S, blink_capacity, 4), dtype=torch.float64, device=dev)
    count, dropped = torch.zeros((S,), dtype=torch.int32, device=dev), torch.zeros((S,), dtype=torch.int32, device=dev)
    flat = lambda t, n: None if t is None else t.reshape(2, S * T, n).contiguous()
    out = default_kernels().eye_gate(
        spec, S, T, state, store, count, dropped, pose_valid=pose_valid,
        reproj_rms=reproj_rms.contiguous() if spec.max_reproj_px is not None else None,
        inliers=inliers.contiguous() if spec.min_inliers is not None else None,
        warp=flat(warps, 9) if spec.min_coverage is not None else None, h=flat(h, 2) if spec.head_angles else None,
        contours=eye_contours.contiguous() if spec.blink is not None else None, lengths=lengths, frame_size=frame_size, patch_size=patch_size)
    return {'usable': out['usable'], 'eye_gate_reason': out['reason'], 'eye_openness': out['openness'], 'blink': out['blink'],
            'blinks': store, 'blink_count': count, 'blink_dropped': dropped, 'gate_state': state}


def render_overlay(frames, format='rgb', out_format='nv12', matrix='bt601', markers=None, heat=None, inset=None, frame_valid=None, out=None):
    """The tracking overlay on the device, stand-alone: frames uint8 [N, ...] in `format` ('rgb' | 'bgr' [N, IH, IW, 3 | 4], 'rgba',
    'bgra', 'nv12' | 'i420' [N, IH*3/2, IW], 'yuyv' [N, IH, IW, 2]) -> the annotated frames, uint8 [N, IH, IW, 3] for out_format 'rgb' |
    'bgr' or [N, IH*3/2, IW] for 'nv12' | 'i420' (IH and IW even).  One launch (eve_overlay_render), bit for bit tests/overlay_ref.py.
      markers      None or a dict: centres float32 [N, M, 2] (x, y), table int32 [M, 4] tensor or nested lists of (r_fill, r_outline,
                   fill 0xRRGGBB, outline 0xRRGGBB), valid None or uint8 [N, M], sx, sy (default 1: the centres are output pixels)
      heat         None, a float32 [N, HH, HW] tensor, or a dict: heat, color (r, g, b) (default red), amax 0..255 (default 128)
      inset        None, a uint8 [N, h, w, 3] RGB tensor (drawn flush in the bottom-right corner), or a dict: inset, xy (x0, y0),
                   zoom 1..4, mirror
      frame_valid  None or uint8 [N]: a 0 gives the converted capture with no layer drawn
    Not offered: the reference's residual lines from an estimate to the ground truth, its legend text, gaze-ray arrows on the eye
    image, row pitches, 10-bit surfaces, a gradient."""
    from .kernels import pixel_format_shape
    kw = {}
    if markers is not None:
        unknown = set(markers) - {'centres', 'table', 'valid', 'sx', 'sy'}
        if unknown or 'centres' not in markers or 'table' not in markers:
            raise ValueError('render_overlay: markers needs centres and table and may hold valid, sx, sy; got %s' % sorted(markers))
        table = markers['table']
        if not torch.is_tensor(table):
            table = torch.tensor(table, dtype=torch.int32).reshape(-1, 4).to(frames.device)
        kw.update(centres=markers['centres'], marker_table=table, marker_valid=markers.get('valid'), sx=float(markers.get('sx', 1.0)),
                  sy=float(markers.get('sy', 1.0)))
    if heat is not None:
        h = heat if isinstance(heat, dict) else {'heat': heat}
        if set(h) - {'heat', 'color', 'amax'} or 'heat' not in h:
            raise ValueError('render_overlay: heat needs heat and may hold color, amax; got %s' % sorted(h))
        kw.update(heat=h['heat'], heat_color=_color(h.get('color', (255, 0, 0)), 'render_overlay: heat color'), amax=h.get('amax', 128))
    if inset is not None:
        p = inset if isinstance(inset, dict) else {'inset': inset}
        if set(p) - {'inset', 'xy', 'zoom', 'mirror'} or 'inset' not in p:
            raise ValueError('render_overlay: inset needs inset and may hold xy, zoom, mirror; got %s' % sorted(p))
        zoom, xy = int(p.get('zoom', 1)), p.get('xy')
        if xy is None:
            if not torch.is_tensor(p['inset']) or p['inset'].dim() != 4:
                raise ValueError('render_overlay: inset must be a uint8 tensor [N, h, w, 3]')
            try:
                IH, IW, _ = pixel_format_shape(frames, {'rgba': 'rgb', 'bgra': 'bgr'}.get(format, format), lead=1)
            except TypeError as e:
                raise ValueError('render_overlay: %s' % e)
            xy = (IW - zoom * int(p['inset'].shape[2]), IH - zoom * int(p['inset'].shape[1]))
        kw.update(inset=p['inset'], inset_xy=xy, zoom=zoom, mirror=bool(p.get('mirror', False)))
    return default_kernels().overlay_render(frames, format, out_format, matrix, frame_valid=frame_valid, out=out, **kw)


class DevicePrefetcher(object):
    """Iterates `iterable` (dicts of CPU tensors, e.g. a DataLoader) and yields the same dicts on `device`.

    A worker thread pulls the next batch, copies pageable tensors into pinned staging buffers (allocated once per
    key / shape and reused; tensors that are already pinned -- DataLoader(pin_memory=True) -- are sent as they are) and
    enqueues the host-to-device copies on a dedicated copy stream, `depth` batches ahead of the consumer; the consumer's
    stream waits on the copy's event, never on the host.  Non-tensor entries pass through."""

    def __init__(self, iterable, device='cuda', depth=2):
        self.iterable = iterable
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.depth = max(1, int(depth))
        self.stream = torch.cuda.Stream(device=self.device)
        self._pinned = [dict() for _ in range(self.depth + 2)]     # staging slots, reused round-robin
        self._slot_events = [None] * len(self._pinned)             # the copy event of the batch last staged from each slot

    def _stage(self, batch, index):
        slot = self._pinned[index]
        # the host must not overwrite a pinned buffer whose host-to-device copy is still queued (the consumer only waits
        # stream-side, so the host can run ahead of the device): wait for this slot's previous copy
        if self._slot_events[index] is not None:
            self._slot_events[index].synchronize()
        out = {}
        with torch.cuda.stream(self.stream):
            for k, v in batch.items():
                if not isinstance(v, torch.Tensor):
                    out[k] = v
                    continue
                src = v
                if not v.is_pinned():
                    buf = slot.get(k)
                    if buf is None or buf.shape != v.shape or buf.dtype != v.dtype:
                        buf = slot[k] = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                    buf.copy_(v)                                   # (memcpy: releases the GIL)
                    src = buf
                out[k] = src.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._slot_events[index] = ev
        return out, ev

    def __iter__(self):
        import queue
        import threading
        q = queue.Queue(maxsize=self.depth)
        done = object()

        def worker():
            try:
                torch.cuda.set_device(self.device)
                for i, batch in enumerate(self.iterable):
                    q.put(self._stage(batch, i % len(self._pinned)))
                q.put(done)
            except BaseException as e:                              # surface loader errors in the consumer
                q.put(e)

        t = threading.Thread(target=worker, daemon=True)
        t.start()
        while True:
            item = q.get()
            if item is done:
                break
            if isinstance(item, BaseException):
                raise item
            out, ev = item
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for v in out.values():
                if isinstance(v, torch.Tensor):
                    v.record_stream(cur)
            yield out
        t.join()
