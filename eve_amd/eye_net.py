"""EyeNet drop-in: per-eye, per-frame ResNet-18(InstanceNorm) encoder -> GRU -> gaze / pupil heads,
computed by the gfx950 HIP kernels of libeve_hip.so.

Mirrors /root/reference/src/models/eye_net.py:
  * constructor signature `EyeNet()` (:38) reading the config singleton, same sub-module / parameter
    names, so `state_dict()` keys equal the reference's (checkpoints split per first prefix by
    src/core/checkpoint_manager.py:56-67 and released weights load with strict=True);
  * `forward(input_dict, output_dict, side, previous_output_dict=None) -> None` (:98) writing
    `<side>_g_initial`, `<side>_pupil_size`, `<side>_eye_rnn_states_0` into `output_dict` and reading
    the previous state from `previous_output_dict` (:116-133); frozen => detached gaze (:149-150);
  * same error behaviour: ValueError for an unknown RNN type (:72), KeyError for missing dict entries.

In addition `forward_sequence` runs all T steps and both eyes of a clip batch in ONE pass: InstanceNorm
has no cross-sample coupling, so folding T and left/right into the image batch is numerically the same
as the reference's per-time-step loop (src/models/eve.py:91-111); only the GRU is sequential, and that
runs as one persistent scan kernel.

The nn.Conv2d / nn.Linear / nn.GRUCell objects below are PARAMETER HOLDERS (names, shapes, init); their
ATen forward is never called.
"""
import math
import os

import torch
from torch import nn

from . import ops
from .config import get_config
from .kernels import (ACT_NONE, ACT_RELU, ACT_SELU, ACT_TANH, HALF_DTYPES, YUV_MATRICES, default_kernels, dispatch_flag, pad_channels,
                      pixel_format_shape)
from .ops import PackedWeight

half_pi = 0.5 * math.pi


def _wants_grad(t):
    return torch.is_grad_enabled() and t.dtype.is_floating_point and t.requires_grad


EYE_PATCH_KEYS = ('left_eye_patch', 'right_eye_patch')
EYE_CAMERA_KEYS = ('camera_frame', 'left_eye_warp', 'right_eye_warp')
# the frame key of a camera form and its pixel format: a batch holds exactly one (camera_frame is RGB(A), the others are what
# cameras and decoders deliver -- kernels.pixel_format_shape has the layouts)
EYE_FRAME_KEYS = {'camera_frame': 'rgb', 'camera_frame_bgr': 'bgr', 'camera_frame_nv12': 'nv12', 'camera_frame_i420': 'i420',
                  'camera_frame_yuyv': 'yuyv'}
# one more frame key: the frame as a decoder's or capture API's surface lies in memory, uint8 [B, T, rows, pitch] or [B, T, frame_bytes],
# read through EyeNet.camera_layout (a data.SurfaceLayout: pitch, coded rows, crop, NV21 / YV12 / UYVY / P010 / pitched BGRA ...)
EYE_SURFACE_KEY = 'camera_surface'
EYE_LENS_KEY = 'camera_lens'                 # optional with the camera form: raw frames of a camera with lens distortion
EYE_POSE_KEY = 'eye_pose'                    # the pose form: camera_frame + one packed row per frame (data.eye_pose)
# what eye_pose_batch derives from the rows -- a batch holds the rows or these, never both
FACE_LANDMARKS_KEY = 'face_landmarks'        # the face-landmark form: camera_frame + 2-D landmarks [B, T, L, 2 | 3] per frame ...
FACE_RIG_KEY = 'face_rig'                    # ... + one row per sequence [B, 12 + 3L] (data.face_rig): the head pose is solved on the device
FACE_LANDMARKS_RAW_KEY = 'face_landmarks_raw'  # in place of face_landmarks: pixels of the RAW frame, undistorted on the device by camera_lens' rows
EYE_POSE_DERIVED = ('head_R', 'left_o', 'right_o', 'left_R', 'right_R', 'left_eye_warp', 'right_eye_warp', 'left_h', 'right_h', 'pose_valid')
# what the face-landmark form adds to them
FACE_DERIVED = ('head_t', 'face_reproj_rms', 'face_inliers')


def has_pose_form(batch):
    """True for a batch whose eye normalisation is derived on the device (eye_pose, or face_landmarks + face_rig): its result
    carries pose_valid."""
    return EYE_POSE_KEY in batch or FACE_LANDMARKS_KEY in batch or FACE_LANDMARKS_RAW_KEY in batch


def face_landmarks_key(batch):
    """face_landmarks or face_landmarks_raw, whichever the batch holds, or None; both raise ValueError."""
    if FACE_LANDMARKS_KEY in batch and FACE_LANDMARKS_RAW_KEY in batch:
        raise ValueError('a batch holds %s (pixels of the undistorted image) or %s (pixels of the raw frame), not both' % (
            FACE_LANDMARKS_KEY, FACE_LANDMARKS_RAW_KEY))
    return FACE_LANDMARKS_KEY if FACE_LANDMARKS_KEY in batch else FACE_LANDMARKS_RAW_KEY if FACE_LANDMARKS_RAW_KEY in batch else None


def camera_frame_key(batch):
    """The one frame key of EYE_FRAME_KEYS (or EYE_SURFACE_KEY) the batch holds, or None; two of them raise ValueError."""
    found = [k_ for k_ in tuple(EYE_FRAME_KEYS) + (EYE_SURFACE_KEY,) if k_ in batch]
    if len(found) > 1:
        raise ValueError('a batch holds one camera frame key, found %s' % ', '.join(found))
    return found[0] if found else None


def _camera_frame(batch):
    key = camera_frame_key(batch)
    frames = batch[key]
    if key == EYE_SURFACE_KEY:                   # (its size is checked against EyeNet.camera_layout where the patches are cut)
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() < 3:
            raise TypeError('%s must be uint8 [B, T, rows, pitch] or [B, T, frame_bytes], got %s %s' % (
                key, getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ()))))
        return frames
    if key != 'camera_frame':
        pixel_format_shape(frames, EYE_FRAME_KEYS[key], lead=2, name=key)
        return frames
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[4] not in (3, 4):
        raise TypeError('camera_frame must be uint8 [B, T, IH, IW, 3 | 4], got %s %s' % (
            getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ()))))
    return frames


def _camera_lens(batch, frames):
    if EYE_LENS_KEY in batch:
        lens = batch[EYE_LENS_KEY]
        if not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) != tuple(frames.shape[:2]) + (12,):
            raise TypeError('%s must be float32 %s, got %s %s' % (EYE_LENS_KEY, tuple(frames.shape[:2]) + (12,),
                                                                   getattr(lens, 'dtype', type(lens)), tuple(getattr(lens, 'shape', ()))))


def eye_input(batch):
    """The tensor that carries a batch's [B, T] and its device: left_eye_patch, or camera_frame when the eyes come as whole
    camera frames plus per-eye homographies (the warp form) or plus eye_pose, float32 [B, T, 18] rows from data.eye_pose (the
    pose form: the homographies, <side>_R, <side>_o, <side>_h and head_R are derived on the device -- eye_pose_batch).  Raises
    on a batch that holds two forms, half of one, eye_pose next to a key it derives, or tensors of the wrong dtype or shape for
    the camera forms.  A third camera form takes the head pose from the face tracker's 2-D landmarks: camera_frame +
    face_landmarks, float32 [B, T, L, 2 | 3] = pixel (u, v[, w]) of the undistorted image, + face_rig, float32 [B, 12 + 3L] rows from
    data.face_rig, one per sequence (the face-landmark form: eve_face_pose_solve solves head_R and head_t on the device and
    the pose form's normalisation continues from them -- eye_pose_batch).  It is refused beside eye_pose, patches or a derived
    key; half of the pair raises ValueError, a wrong dtype or shape TypeError.  face_landmarks_raw, same shape, stands in for
    face_landmarks with pixels of the RAW frame (what a tracker fed the raw frame reports): it REQUIRES camera_lens, whose rows
    undistort both the pixels and the points (ValueError without it, and with both landmark keys); face_landmarks + camera_lens
    keeps meaning landmarks of the undistorted image.  All camera forms may carry camera_lens, float32 [B, T, 12] (data.camera_lens): one camera per frame,
    for both eyes.  In both, camera_frame may be replaced by ONE of camera_frame_bgr [B, T, IH, IW, 3 | 4], camera_frame_nv12 /
    camera_frame_i420 [B, T, IH*3/2, IW] or camera_frame_yuyv [B, T, IH, IW, 2] (EYE_FRAME_KEYS; two frame keys raise ValueError,
    odd sizes too): that tensor is then returned -- its shape[:2] and device are the batch's whatever the format.  camera_surface,
    uint8 [B, T, rows, pitch] or [B, T, frame_bytes], is one more such key: the frame as a decoder's surface lies in memory, read
    through EyeNet.camera_layout."""
    lm_key = face_landmarks_key(batch)
    if lm_key is not None or FACE_RIG_KEY in batch:
        if lm_key is None or FACE_RIG_KEY not in batch:
            raise ValueError('the face-landmark form needs %s and %s: found only %s' % (
                lm_key or FACE_LANDMARKS_KEY, FACE_RIG_KEY, lm_key or FACE_RIG_KEY))
        clash = [k_ for k_ in (EYE_POSE_KEY,) + EYE_PATCH_KEYS + EYE_POSE_DERIVED + FACE_DERIVED if k_ in batch]
        if clash:
            raise ValueError('%s + %s derive %s and stand in for %s and %s: found %s beside them' % (
                lm_key, FACE_RIG_KEY, ', '.join(EYE_POSE_DERIVED + FACE_DERIVED), EYE_POSE_KEY, ' / '.join(EYE_PATCH_KEYS),
                ', '.join(clash)))
        if camera_frame_key(batch) is None:
            raise ValueError('%s goes with camera_frame: the patches are cut from it' % lm_key)
        if lm_key == FACE_LANDMARKS_RAW_KEY and EYE_LENS_KEY not in batch:
            raise ValueError('%s holds pixels of the raw frame and needs %s, whose rows undistort both the pixels and the points '
                             '(landmarks of an undistorted image go in as %s)' % (lm_key, EYE_LENS_KEY, FACE_LANDMARKS_KEY))
        frames = _camera_frame(batch)
        lm, rig = batch[lm_key], batch[FACE_RIG_KEY]
        B, T = frames.shape[:2]
        if (not torch.is_tensor(lm) or lm.dtype != torch.float32 or lm.dim() != 4 or tuple(lm.shape[:2]) != (B, T)
                or not 4 <= lm.shape[2] <= 68 or lm.shape[3] not in (2, 3)):
            raise TypeError('%s must be float32 %s with 4 <= L <= 68, got %s %s' % (
                lm_key, (B, T, 'L', '2 | 3'), getattr(lm, 'dtype', type(lm)), tuple(getattr(lm, 'shape', ()))))
        if not torch.is_tensor(rig) or rig.dtype != torch.float32 or tuple(rig.shape) != (B, 12 + 3 * lm.shape[2]):
            raise TypeError('%s must be float32 %s (one row per sequence), got %s %s' % (
                FACE_RIG_KEY, (B, 12 + 3 * lm.shape[2]), getattr(rig, 'dtype', type(rig)), tuple(getattr(rig, 'shape', ()))))
        _camera_lens(batch, frames)
        return frames
    if EYE_POSE_KEY in batch:
        clash = [k_ for k_ in EYE_PATCH_KEYS + EYE_POSE_DERIVED if k_ in batch]
        if clash:
            raise ValueError('%s derives %s and stands in for %s: found %s beside it' % (
                EYE_POSE_KEY, ', '.join(EYE_POSE_DERIVED), ' / '.join(EYE_PATCH_KEYS), ', '.join(clash)))
        if camera_frame_key(batch) is None:
            raise ValueError('%s goes with camera_frame: the patches are cut from it' % EYE_POSE_KEY)
        frames = _camera_frame(batch)
        pose = batch[EYE_POSE_KEY]
        if not torch.is_tensor(pose) or pose.dtype != torch.float32 or tuple(pose.shape) != tuple(frames.shape[:2]) + (18,):
            raise TypeError('%s must be float32 %s, got %s %s' % (EYE_POSE_KEY, tuple(frames.shape[:2]) + (18,),
                                                                   getattr(pose, 'dtype', type(pose)), tuple(getattr(pose, 'shape', ()))))
        _camera_lens(batch, frames)
        return frames
    has_patch = [k_ for k_ in EYE_PATCH_KEYS if k_ in batch]
    frame_key = camera_frame_key(batch)
    has_cam = [k_ for k_ in EYE_CAMERA_KEYS if k_ in batch or (k_ == 'camera_frame' and frame_key is not None)]
    if has_patch and has_cam:
        raise ValueError('give the eyes either as %s or as %s, not both (found %s)' % (
            ' / '.join(EYE_PATCH_KEYS), ' / '.join(EYE_CAMERA_KEYS), ', '.join(has_patch + [frame_key if k_ == 'camera_frame' else k_
                                                                                             for k_ in has_cam])))
    if not has_cam:
        if EYE_LENS_KEY in batch:
            raise ValueError('%s goes with %s: pre-cut patches were cut from an undistorted frame already' % (
                EYE_LENS_KEY, ' / '.join(EYE_CAMERA_KEYS)))
        return batch['left_eye_patch']
    if len(has_cam) != len(EYE_CAMERA_KEYS):
        raise ValueError('the camera form needs %s: missing %s' % (
            ', '.join(EYE_CAMERA_KEYS), ', '.join(k_ for k_ in EYE_CAMERA_KEYS if k_ not in has_cam)))
    frames = _camera_frame(batch)
    for k_ in EYE_CAMERA_KEYS[1:]:
        w = batch[k_]
        if not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != tuple(frames.shape[:2]) + (3, 3):
            raise TypeError('%s must be float32 %s, got %s %s' % (k_, tuple(frames.shape[:2]) + (3, 3), getattr(w, 'dtype', type(w)),
                                                                   tuple(getattr(w, 'shape', ()))))
    _camera_lens(batch, frames)
    return frames


def _face_landmark_batch(batch, config, face_state, reset, lengths, huber_px=None):
    """eye_pose_batch for camera_frame + face_landmarks + face_rig: ONE eve_face_pose_solve launch (every sequence one wavefront,
    every frame warm-started from the one before, frame 0 from face_state where that holds a pose) and ONE
    eve_eye_pose_normalize_rt launch that continues from the float32 head_R / head_t just written.  With face_landmarks_raw
    (camera_lens' rows undistort the points inside the launch) or huber_px (a Huber loss) the launch is eve_face_pose_solve_ex
    and the copy gains face_inliers, uint8 [B, T]."""
    from . import data
    frames = eye_input(batch)
    B, T = frames.shape[:2]
    k = default_kernels()
    rig = batch[FACE_RIG_KEY].contiguous()
    lm_key = face_landmarks_key(batch)
    huber_px = data.check_huber_px(huber_px, 'face_huber_px')
    inliers = None
    if lm_key == FACE_LANDMARKS_RAW_KEY or huber_px is not None:
        lens = batch[EYE_LENS_KEY].contiguous() if lm_key == FACE_LANDMARKS_RAW_KEY else None
        head_R, head_t, rms, solved, inliers = k.face_pose_solve_ex(batch[lm_key].contiguous(), rig, lens, huber_px, lengths, face_state, reset)
    else:
        head_R, head_t, rms, solved = k.face_pose_solve(batch[lm_key].contiguous(), rig, lengths, face_state, reset)
    o, R, warp, h, valid = k.eye_pose_normalize_rt(rig, head_R, head_t, solved, data.eye_patch_hw(config))
    d = {k_: v for k_, v in batch.items() if k_ not in (lm_key, FACE_RIG_KEY)}
    d['head_R'], d['head_t'], d['face_reproj_rms'] = head_R, head_t, rms
    if inliers is not None:
        d['face_inliers'] = inliers
    for e, side in enumerate(('left', 'right')):
        d[side + '_o'] = o[e].view(B, T, 3)
        d[side + '_R'] = R[e].view(B, T, 3, 3)
        d[side + '_eye_warp'] = warp[e].view(B, T, 3, 3)
        d[side + '_h'] = h[e].view(B, T, 2)
    d['pose_valid'] = valid.view(2, B, T).permute(1, 2, 0) != 0
    return d


def eye_pose_batch(batch, config=None, face_state=None, reset=None, lengths=None, huber_px=None):
    """The pose form turned into the warp form: a batch without eye_pose comes back as it is; one with it is checked (eye_input)
    and copied, and in the copy eye_pose is replaced by what ONE eve_eye_pose_normalize launch derives from the rows for the
    config's eyes_size: head_R [B, T, 3, 3], <side>_o [B, T, 3], <side>_R [B, T, 3, 3], <side>_eye_warp [B, T, 3, 3] (inv(W): what
    the eye-warp kernels take), <side>_h [B, T, 2] and pose_valid, bool [B, T, 2] (left, right).  An eye whose pose is not usable
    (a NaN, a head behind the camera, ...) has pose_valid False, a zero warp -- so a black patch -- R = I, o = 0 and h = 0;
    pose_valid is reported and folded into nothing.  Every entry point that takes the eyes calls this once, before anything
    reads a derived key; the copy holds no eye_pose, so the modules below it see the warp form.
    The face-landmark form (camera_frame + face_landmarks + face_rig) is turned into the warp form the same way, with the head
    pose solved on the device first (_face_landmark_batch): the copy additionally gains head_t [B, T, 3] and face_reproj_rms
    [B, T] (pixels), and pose_valid is False for both eyes of a frame with no solution.  face_state: None (every sequence starts
    cold) or the float64 [B, 13] carried pose of an EVEStream, updated in place; reset, lengths: None or int32 [B] device tensors
    (flagged sequences start cold; frames past a sequence's count are not solved).  The three are read by this form only.
    face_landmarks_raw in place of face_landmarks holds pixels of the RAW frame and needs camera_lens, whose rows undistort the
    points inside the solve's launch; huber_px (EyeNet.face_huber_px: None or k > 0 pixels) gives the solve a Huber loss.  With
    either the copy gains face_inliers, uint8 [B, T] (include/eve_hip.h eve_face_pose_solve_ex)."""
    if face_landmarks_key(batch) is not None or FACE_RIG_KEY in batch:
        return _face_landmark_batch(batch, config, face_state, reset, lengths, huber_px)
    if EYE_POSE_KEY not in batch:
        return batch
    from . import data
    frames = eye_input(batch)
    B, T = frames.shape[:2]
    head_R, o, R, warp, h, valid = default_kernels().eye_pose_normalize(batch[EYE_POSE_KEY].reshape(B * T, 18).contiguous(),
                                                                        data.eye_patch_hw(config))
    d = {k_: v for k_, v in batch.items() if k_ != EYE_POSE_KEY}
    d['head_R'] = head_R.view(B, T, 3, 3)
    for e, side in enumerate(('left', 'right')):
        d[side + '_o'] = o[e].view(B, T, 3)
        d[side + '_R'] = R[e].view(B, T, 3, 3)
        d[side + '_eye_warp'] = warp[e].view(B, T, 3, 3)
        d[side + '_h'] = h[e].view(B, T, 2)
    d['pose_valid'] = valid.view(2, B, T).permute(1, 2, 0) != 0
    return d


def default_compute_dtype():
    name = os.environ.get('EVE_AMD_DTYPE', 'fp32').lower()
    if name in ('bf16', 'bfloat16'):
        return torch.bfloat16
    if name in ('fp16', 'float16', 'half'):
        return torch.float16
    if name in ('fp32', 'float32', 'f32'):
        return torch.float32
    raise ValueError('EVE_AMD_DTYPE must be fp32, bf16 or fp16, got %r' % name)


class _Block(nn.Module):
    """Parameter holder for one torchvision BasicBlock (conv1, conv2, optional downsample.0)."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.stride = stride
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False),
                                            nn.InstanceNorm2d(cout))


class _ResNet18IN(nn.Module):
    """Parameter holder with torchvision ResNet-18 names (conv1, layer1..4, fc)."""

    def __init__(self, num_classes):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        cin = 64
        for li, (cout, stride) in enumerate([(64, 1), (128, 2), (256, 2), (512, 2)], start=1):
            setattr(self, 'layer%d' % li, nn.Sequential(_Block(cin, cout, stride), _Block(cout, cout, 1)))
            cin = cout
        self.fc = nn.Linear(512, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    def blocks(self):
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(self, 'layer%d' % li)):
                yield 'layer%d.%d' % (li, bi), blk


class EyeNet(nn.Module):
    def __init__(self):
        super(EyeNet, self).__init__()
        config = get_config()
        self.config = config
        self.compute_dtype = default_compute_dtype()
        nf = (config.eye_net_rnn_num_features if config.eye_net_use_rnn
              else config.eye_net_static_num_features)
        self.num_features = nf
        self.cnn_layers = _ResNet18IN(nf)
        self.fc_common = nn.Sequential(
            nn.Linear(nf + (2 if config.eye_net_use_head_pose_input else 0), nf),
            nn.SELU(inplace=True),
            nn.Linear(nf, nf),
        )
        if config.eye_net_use_rnn:
            cells = []
            for _ in range(config.eye_net_rnn_num_cells):
                kind = config.eye_net_rnn_type
                n = config.eye_net_rnn_num_features
                if kind == 'RNN':
                    cells.append(nn.RNNCell(input_size=n, hidden_size=n))
                elif kind == 'LSTM':
                    cells.append(nn.LSTMCell(input_size=n, hidden_size=n))
                elif kind == 'GRU':
                    cells.append(nn.GRUCell(input_size=n, hidden_size=n))
                else:
                    raise ValueError('Unknown RNN type for EyeNet: %s' % kind)
            self.rnn_cells = nn.ModuleList(cells)
        else:
            self.static_fc = nn.Sequential(nn.Linear(nf, nf), nn.SELU(inplace=True))
        self.fc_to_gaze = nn.Sequential(
            nn.Linear(nf, nf), nn.SELU(inplace=True), nn.Linear(nf, 2, bias=False), nn.Tanh())
        self.fc_to_pupil = nn.Sequential(
            nn.Linear(nf, nf), nn.SELU(inplace=True), nn.Linear(nf, 1), nn.ReLU(inplace=True))
        nn.init.zeros_(self.fc_to_gaze[-2].weight)
        self._packs = None
        self._packs_key = None

    # ------------------------------------------------------------------ packed weights
    def invalidate_packs(self):
        """Call after the parameters were updated behind torch's back (the fused Adam kernel)."""
        self._packs = None

    def _get_packs(self):
        dt = self.compute_dtype
        key = (dt,) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packs is not None and self._packs_key == key:
            return self._packs
        f32 = torch.float32
        P = {}
        cnn = self.cnn_layers
        P['conv1'] = PackedWeight(cnn.conv1.weight, dt, cin_pad=pad_channels(3, dt), want_ihwo=False, defer=True)
        for name, blk in cnn.blocks():
            P[name + '.conv1'] = PackedWeight(blk.conv1.weight, dt, defer=True)
            P[name + '.conv2'] = PackedWeight(blk.conv2.weight, dt, defer=True)
            if blk.downsample is not None:
                P[name + '.downsample.0'] = PackedWeight(blk.downsample[0].weight, dt, defer=True)
        PackedWeight.pack_many(list(P.values()), dt)          # all trunk weights in one launch
        P['conv1.dgrad'] = ops.StemDgradPack(cnn.conv1.weight, dt)   # packed only when patches require a gradient
        # the tail (linears + GRU) always runs in float32: < 0.03 % of the FLOPs, and it carries the recurrence
        T = {}
        T['fc'] = PackedWeight(cnn.fc.weight, f32, defer=True)
        T['fc_common.0'] = PackedWeight(self.fc_common[0].weight, f32,
                                        cin_pad=pad_channels(self.fc_common[0].in_features, f32), defer=True)
        T['fc_common.2'] = PackedWeight(self.fc_common[2].weight, f32, defer=True)
        if self.config.eye_net_use_rnn:
            for i, cell in enumerate(self.rnn_cells):
                T['rnn.%d.ih' % i] = PackedWeight(cell.weight_ih, f32, defer=True)
                if i == 0 and self.config.eye_net_rnn_type == 'GRU':        # W_hh and its transpose for ops.EyeTailLossFn
                    T['rnn.0.hh'] = PackedWeight(cell.weight_hh, f32, defer=True)
        else:
            T['static_fc.0'] = PackedWeight(self.static_fc[0].weight, f32, defer=True)
        T['fc_to_gaze.0'] = PackedWeight(self.fc_to_gaze[0].weight, f32, defer=True)
        T['fc_to_gaze.2'] = PackedWeight(self.fc_to_gaze[2].weight, f32, cout_pad=4, defer=True)
        T['fc_to_pupil.0'] = PackedWeight(self.fc_to_pupil[0].weight, f32, defer=True)
        T['fc_to_pupil.2'] = PackedWeight(self.fc_to_pupil[2].weight, f32, cout_pad=4, defer=True)
        PackedWeight.pack_many(list(T.values()), f32)
        P.update(T)
        self._packs, self._packs_key = P, key
        return P

    # ------------------------------------------------------------------ trunk
    def _trunk(self, x, P, x_padded=None, patches=None):
        """x: [N, H, W, Cpad] NHWC compute dtype -> [N, 512] float32 (torchvision ResNet._forward_impl).
        x_padded: optional [N, H+6, W+8, 4] bf16 repack for the dedicated stem kernel.
        patches: None, or the float NCHW patch batches x / x_padded were made from (concatenated along the batch), when their
        gradient is wanted: the stem's data gradient (stem_dgrad) is then returned to them."""
        y = self._trunk_layers(x, P, x_padded, patches)
        if hasattr(ops.default_kernels(), 'avgpool_fwd_f32'):
            return ops.AvgPoolF32Fn.apply(y)                  # pool + cast in one launch each way (same bits)
        return ops.cast(ops.AvgPoolFn.apply(y), torch.float32)

    def _trunk_layers(self, x, P, x_padded=None, patches=None):
        """conv1 .. layer4 of the trunk: -> [N, H/32, W/32, 512] NHWC compute dtype."""
        cnn = self.cnn_layers
        blocks, weights = [], []
        for name, blk in cnn.blocks():
            ds = blk.downsample
            blocks.append(((P[name + '.conv1'], P[name + '.conv2'], P[name + '.downsample.0'] if ds is not None else None),
                           blk.stride))
            weights += [blk.conv1.weight, blk.conv2.weight] + ([ds[0].weight] if ds is not None else [])
        if x_padded is not None and x_padded.shape[2] == 136 and x_padded.shape[1] % 4 == 2:
            # 128-wide patches: conv1 -> bn1 -> relu -> maxpool in one launch, inside the trunk node
            if patches is not None:             # (the two patch batches in the node's x / x8 slots: their gradient comes back there)
                assert len(patches) == 2
                P['conv1.dgrad'].get()
                y = ops.ResNetTrunkFn.apply(patches[0], patches[1], x_padded, (P['conv1'], tuple(blocks), P['conv1.dgrad']), 1e-5,
                                            cnn.conv1.weight, *weights)
            else:
                y = ops.ResNetTrunkFn.apply(None, x, x_padded, (P['conv1'], tuple(blocks)), 1e-5, cnn.conv1.weight, *weights)
        else:
            if x_padded is not None:
                y = ops.StemConvFn.apply(x, x_padded, cnn.conv1.weight, P['conv1'])
            else:
                y = ops.conv2d(x, cnn.conv1.weight, None, P['conv1'], stride=2, pad=3)
            if patches is not None:
                y = ops.StemPatchGradFn.apply(y, P['conv1.dgrad'], *patches)
            y = ops.InReluMaxPoolFn.apply(y, 1e-5)      # bn1 -> relu -> maxpool, fused
            y = ops.ResNetTrunkFn.apply(y, None, None, (None, tuple(blocks)), 1e-5, *weights)
        return y

    # ------------------------------------------------------------------ tail: fc -> fc_common -> GRU -> heads
    def _tail(self, feats, head_pose, S, T, h0, P):
        """feats [S*T, 512] float32 ordered (sequence, time); head_pose [S*T, 2] or None; h0: None or one initial
        state per cell ([S, H] tensor, (h, c) pair for LSTM, or None).
        Returns gaze [S*T, 2] (rad), pupil [S*T], states: None or per cell [S, T, H] / ((h) [S, T, H], (c) [S, T, H])."""
        cfg = self.config
        cnn = self.cnn_layers
        k = default_kernels()
        f = ops.linear(feats, cnn.fc.weight, cnn.fc.bias, P['fc'])
        if cfg.eye_net_use_head_pose_input:
            f = torch.cat([f, head_pose.to(f.dtype)], dim=1)
        cin_p = P['fc_common.0'].ohwi.shape[3]
        if f.shape[1] != cin_p:
            f = torch.nn.functional.pad(f, (0, cin_p - f.shape[1]))
        f = ops.linear(f.contiguous(), self.fc_common[0].weight, self.fc_common[0].bias, P['fc_common.0'],
                       act=ACT_SELU)
        f = ops.linear(f, self.fc_common[2].weight, self.fc_common[2].bias, P['fc_common.2'])
        states = None
        if cfg.eye_net_use_rnn:
            # the cells form a stack over depth; cell i at step t reads cell i-1 at step t and its own state at t-1, so
            # each cell is one scan over the whole sequence of its predecessor's outputs (eye_net.py:112-135)
            states = []
            for i, cell in enumerate(self.rnn_cells):
                init = h0[i] if h0 is not None else None
                gi = ops.linear(f, cell.weight_ih, cell.bias_ih, P['rnn.%d.ih' % i])
                H = cell.hidden_size
                kind = cfg.eye_net_rnn_type
                if kind == 'GRU':
                    st = ops.GRUScanFn.apply(gi.view(S, T, 3 * H), cell.weight_hh, cell.bias_hh, init)
                    hs = st
                elif kind == 'RNN':
                    st = ops.RNNScanFn.apply(gi.view(S, T, H), cell.weight_hh, cell.bias_hh, init)
                    hs = st
                else:                                   # LSTM: the state is the (h, c) pair, the output is h
                    h_init, c_init = init if init is not None else (None, None)
                    st = ops.LSTMScanFn.apply(gi.view(S, T, 4 * H), cell.weight_hh, cell.bias_hh, h_init, c_init)
                    hs = st[0]
                states.append(st)
                f = hs.reshape(S * T, H)
        else:
            f = ops.linear(f, self.static_fc[0].weight, self.static_fc[0].bias, P['static_fc.0'], act=ACT_SELU)
        g = ops.linear(f, self.fc_to_gaze[0].weight, self.fc_to_gaze[0].bias, P['fc_to_gaze.0'], act=ACT_SELU)
        g = ops.linear(g, self.fc_to_gaze[2].weight, None, P['fc_to_gaze.2'], act=ACT_TANH)
        gaze = half_pi * g[:, :2]
        p = ops.linear(f, self.fc_to_pupil[0].weight, self.fc_to_pupil[0].bias, P['fc_to_pupil.0'], act=ACT_SELU)
        p = ops.linear(p, self.fc_to_pupil[2].weight, self.fc_to_pupil[2].bias, P['fc_to_pupil.2'], act=ACT_RELU)
        return gaze, p[:, 0], states

    # ------------------------------------------------------------------ train step: tail + losses as one node
    tail_loss_node = None        # None: eve_dispatch_config.tail_loss_node (default on); a test sets True / False on the instance

    def _tail_loss_node_ok(self, batch, T, feats=None):
        cfg = self.config
        if feats is not None and not feats.requires_grad:
            # (frozen trunk + trainable tail: the node takes the tail parameters through `self`, not as autograd inputs, so
            # its outputs would carry no graph -- the per-layer path handles that configuration)
            return False
        if batch['left_h'].requires_grad or batch['right_h'].requires_grad:
            return False                        # the node returns no head-pose gradient: the per-layer path does
        k = default_kernels()
        on = self.tail_loss_node if self.tail_loss_node is not None else bool(dispatch_flag(k, 'tail_loss_node', 1))
        if not (on and hasattr(k, 'tail_outputs_fwd') and torch.is_grad_enabled() and cfg.eye_net_use_rnn and
                cfg.eye_net_rnn_type == 'GRU' and len(self.rnn_cells) == 1 and cfg.eye_net_use_head_pose_input and
                not cfg.eye_net_frozen and self.rnn_cells[0].hidden_size == 128 and self.fc_common[0].in_features == 130 and
                self.cnn_layers.fc.in_features == 512 and T <= 256 and eye_input(batch).is_cuda and
                batch['left_g_tobii'].dtype == torch.float32 and batch['left_h'].dtype == torch.float32):
            return False
        return all(ops._direct_grad_ok(p_) for p_ in ops.EyeTailLossFn.tail_parameters(self))

    def loss_terms_sequence(self, batch, config=None):
        """The EyeNet train step's forward: whole clips of both eyes -> the loss terms of eve.py:286-325 that carry weight in
        eye_net.json and their weighted sum (:234-265) -- what losses.eyenet_loss_terms(self.forward_sequence(batch), ...) returns,
        with the tail and the losses as ONE autograd node (ops.EyeTailLossFn) when the configuration is the product one
        (train.eyenet_trainer: one GRU cell, head-pose input, parameters in the trainer's flat buffers); any other
        configuration takes the per-layer path.  Also returns the predictions (detached) under the forward_sequence keys."""
        from . import losses
        config = config if config is not None else self.config
        batch = eye_pose_batch(batch, self.config, huber_px=self.face_huber_px)
        P = self._get_packs()
        feats, B, T = self._sequence_features(batch, P)
        self.last_tail_path = 'node' if self._tail_loss_node_ok(batch, T, feats) else 'layers'
        if self.last_tail_path == 'layers':
            out = self._sequence_tail(feats, batch, B, T, None, P)
            terms = losses.eyenet_loss_terms(out, batch, config)
            terms.update({k_: v.detach() for k_, v in out.items() if torch.is_tensor(v)})
            return terms
        tgt = tuple(batch[k_] for k_ in ('left_g_tobii', 'right_g_tobii', 'left_g_tobii_validity', 'right_g_tobii_validity',
                                         'left_p', 'right_p', 'left_p_validity', 'right_p_validity'))
        packs = tuple(P[n] for n in ('fc', 'fc_common.0', 'fc_common.2', 'rnn.0.ih', 'rnn.0.hh', 'fc_to_gaze.0', 'fc_to_gaze.2',
                                     'fc_to_pupil.0', 'fc_to_pupil.2'))
        t = ops.EyeTailLossFn.apply(feats, batch['left_h'], batch['right_h'], tgt, float(config.loss_coeff_g_ang_initial),
                                    float(config.loss_coeff_pupil_size), self, packs, B, T)
        gaze, pupil, hs = t[5], t[6], t[7]
        BT = B * T
        return {'loss_ang_left_g_initial': t[0], 'loss_l1_left_pupil_size': t[1], 'loss_ang_right_g_initial': t[2],
                'loss_l1_right_pupil_size': t[3], 'full_loss': t[4],
                'left_g_initial': gaze[:BT].view(B, T, 2), 'right_g_initial': gaze[BT:].view(B, T, 2),
                'left_pupil_size': pupil[:BT].view(B, T), 'right_pupil_size': pupil[BT:].view(B, T),
                'left_eye_rnn_states_0': hs[:B], 'right_eye_rnn_states_0': hs[B:]}

    # ------------------------------------------------------------------ reference per-step contract
    def forward(self, input_dict, output_dict, side, previous_output_dict=None):
        key = side + '_eye_patch'
        image = output_dict[key] if key in output_dict else input_dict[key]
        P = self._get_packs()
        dt = self.compute_dtype
        if _wants_grad(image):
            # the patch's gradient from the stem's data-gradient kernel, like the clip path's (not through the padded NHWC copy)
            x = default_kernels().nchw_to_nhwc(image.detach().contiguous().float(), dt, pad_channels(image.shape[1], dt))
            feats = self._trunk(x, P, patches=(image,))
        else:
            x = ops.ToNHWCFn.apply(image, dt, pad_channels(image.shape[1], dt))
            feats = self._trunk(x, P)
        head_pose = input_dict[side + '_h'] if self.config.eye_net_use_head_pose_input else None
        h0 = None
        ncell = len(self.rnn_cells) if self.config.eye_net_use_rnn else 0
        if ncell and previous_output_dict is not None:
            h0 = [previous_output_dict[side + '_eye_rnn_states_%d' % i] for i in range(ncell)]
        B = image.shape[0]
        gaze, pupil, states = self._tail(feats, head_pose, B, 1, h0, P)
        for i in range(ncell):
            st = states[i]
            output_dict[side + '_eye_rnn_states_%d' % i] = tuple(s_[:, 0] for s_ in st) if isinstance(st, tuple) else st[:, 0]
        output_dict[side + '_g_initial'] = gaze
        output_dict[side + '_pupil_size'] = pupil.reshape(-1)
        if self.config.eye_net_frozen:
            output_dict[side + '_g_initial'] = output_dict[side + '_g_initial'].detach()

    # ------------------------------------------------------------------ whole clips, both eyes, one pass
    # The YUV -> RGB matrix of camera_frame_nv12 / _i420 / _yuyv batches: 'bt601' (limited range: webcams, OpenCV's cvtColor),
    # 'bt709' (limited range: HD decoders) or 'jfif' (full range: MJPEG).  Anything else raises ValueError at use.
    yuv_matrix = 'bt601'
    # How camera_surface batches lie in memory: a data.SurfaceLayout (format, visible size, pitch, coded rows, crop origin, plane
    # offsets).  A camera_surface batch without it raises ValueError.
    camera_layout = None
    # The face-landmark forms' Huber loss: None, or k > 0 in pixels (3 suits 1 px of landmark noise) -- landmarks further than k from
    # their reprojection are down-weighted by k / distance, so a few confidently wrong ones (a hand, hair) no longer tilt the head.
    # Anything else raises ValueError where a face-landmark batch is used.  An EVEStream captures one graph per value.
    face_huber_px = None

    def forward_sequence(self, batch, initial_states=None):
        """batch: {left,right}_eye_patch [B, T, 3, H, W] float (or uint8 [B, T, H, W, C] decoded frames), {left,right}_h [B, T, 2].
        In place of the two patch keys the batch may hold whole camera frames, camera_frame uint8 [B, T, IH, IW, 3 | 4], and
        {left,right}_eye_warp float32 [B, T, 3, 3], the homographies from a patch pixel to a camera pixel (data.warp_eye_patches):
        the patches, of the config's eyes_size, are then cut on the device.  With camera_lens, float32 [B, T, 12] (data.camera_lens:
        the intrinsics and OpenCV distortion coefficients of the camera behind each frame), camera_frame is the RAW frame and the
        warps refer to the undistorted image the networks were trained on: the cut undistorts as it samples.
        Or the pose form: camera_frame and eye_pose, float32 [B, T, 18] (data.eye_pose), in place of the patches, the warps AND
        {left,right}_h -- eye_pose_batch derives them on the device.
        In every camera form the frames may come as the camera or decoder delivers them, under ONE of camera_frame_bgr,
        camera_frame_nv12, camera_frame_i420, camera_frame_yuyv in place of camera_frame (eye_input has the shapes): the cut then
        converts the taps it reads by the integer matrix self.yuv_matrix names, and equals the cut from the converted RGB frame bit
        for bit (eve_eye_warp_fmt_to_nchw).  Or under camera_surface, uint8 [B, T, rows, pitch] or [B, T, frame_bytes]: the surface
        as it lies in memory -- pitched rows, coded rows, a crop, NV21 / YV12 / UYVY / P010 / pitched BGRA -- read through
        self.camera_layout, a data.SurfaceLayout (eve_eye_warp_surface_to_nchw): the cut equals the one from the de-pitched, cropped,
        byte-linear frame bit for bit, and that copy is never made.  The per-frame forward() takes patches only.
        Returns the B x T x ... tensors eve.py:174-182 would stack: <side>_g_initial [B,T,2],
        <side>_pupil_size [B,T], <side>_eye_rnn_states_<i> [B,T,H] per cell ((h, c) pair of them for LSTM).
        initial_states: {side: h [B,H]} or {side: [per-cell h | (h, c) | None]}."""
        batch = eye_pose_batch(batch, self.config, huber_px=self.face_huber_px)
        P = self._get_packs()
        feats, B, T = self._sequence_features(batch, P)
        return self._sequence_tail(feats, batch, B, T, initial_states, P)

    def _camera_cutters(self, batch):
        """The camera forms' patch cut as closures over the batch's frames, lens rows and pixel format -> (B, T, Hh, Ww, lw, rw,
        to_stem, to_nchw): lw, rw the two eyes' homographies [B*T, 3, 3]; to_stem(w, out) cuts into the stem's packed layout,
        to_nchw(w) to float NCHW patches [B*T, 3, Hh, Ww] in [-1, 1] (EVEStream's overlay inset cuts its patches through it)."""
        k = default_kernels()
        frame_key = camera_frame_key(batch)
        from . import data
        frames = batch[frame_key]
        B, T = frames.shape[:2]
        Hh, Ww = data.eye_patch_hw(self.config)
        flat = frames.reshape((B * T,) + tuple(frames.shape[2:])).contiguous()
        lw, rw = (batch[s_ + '_eye_warp'].reshape(B * T, 3, 3).contiguous() for s_ in ('left', 'right'))
        if frame_key == EYE_SURFACE_KEY:        # a surface as it lies in memory: the taps go through the layout's address rule
            layout, matrix = self.camera_layout, self.yuv_matrix
            if layout is None:
                raise ValueError('%s needs EyeNet.camera_layout, a data.SurfaceLayout that says how the frames lie in memory' % EYE_SURFACE_KEY)
            if matrix not in YUV_MATRICES:
                raise ValueError('EyeNet.yuv_matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), matrix))
            flat, _ = data.surface_frames(frames, layout, 2, name=EYE_SURFACE_KEY)
            lens = batch[EYE_LENS_KEY].reshape(B * T, 12).contiguous() if EYE_LENS_KEY in batch else None
            to_stem = lambda w, out: k.eye_warp_surface_to_stem(flat, w, (Hh, Ww), layout, matrix=matrix, lens=lens, out=out)
            to_nchw = lambda w: k.eye_warp_surface_to_nchw(flat, w, (Hh, Ww), layout, matrix=matrix, lens=lens)
        elif frame_key != 'camera_frame':       # BGR / NV12 / I420 / YUYV: the taps are converted inside the same launch
            fmt, matrix = EYE_FRAME_KEYS[frame_key], self.yuv_matrix
            if matrix not in YUV_MATRICES:
                raise ValueError('EyeNet.yuv_matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), matrix))
            lens = batch[EYE_LENS_KEY].reshape(B * T, 12).contiguous() if EYE_LENS_KEY in batch else None
            to_stem = lambda w, out: k.eye_warp_fmt_to_stem(flat, w, (Hh, Ww), fmt, matrix=matrix, lens=lens, out=out)
            to_nchw = lambda w: k.eye_warp_fmt_to_nchw(flat, w, (Hh, Ww), fmt, matrix=matrix, lens=lens)
        elif EYE_LENS_KEY in batch:             # raw frames: the lens kernels, one camera per frame for both eyes
            lens = batch[EYE_LENS_KEY].reshape(B * T, 12).contiguous()
            to_stem = lambda w, out: k.eye_warp_lens_u8_to_stem(flat, w, lens, (Hh, Ww), out=out)
            to_nchw = lambda w: k.eye_warp_lens_u8_to_nchw(flat, w, lens, (Hh, Ww))
        else:
            to_stem = lambda w, out: k.eye_warp_u8_to_stem(flat, w, (Hh, Ww), out=out)
            to_nchw = lambda w: k.eye_warp_u8_to_nchw(flat, w, (Hh, Ww))
        return B, T, Hh, Ww, lw, rw, to_stem, to_nchw

    def _sequence_features(self, batch, P):
        """Both eyes' clips through the trunk: -> feats [2*B*T, 512] float32 (left clips' frames, then the right ones'), B, T."""
        k = default_kernels()
        dt = self.compute_dtype
        x = x_padded = None
        frame_key = camera_frame_key(batch)
        if eye_input(batch) is batch.get(frame_key):
            # whole camera frames and one homography per eye and frame: cut, normalise and lay out in one launch per eye --
            # straight into the stem's packed layout where the uint8 patches below go there, else to float NCHW patches
            frames = batch[frame_key]
            B, T, Hh, Ww, lw, rw, to_stem, to_nchw = self._camera_cutters(batch)
            C, flat = 3, frames
            if dt in HALF_DTYPES and Hh % 4 == 0 and Ww == 128:
                x_padded = torch.empty((2 * B * T, Hh + 6, Ww + 8, 4), dtype=dt, device=frames.device)
                to_stem(lw, x_padded[:B * T])
                to_stem(rw, x_padded[B * T:])
                left = right = flat                 # (no float patches: nothing below reads them)
            else:
                left = to_nchw(lw).view(B, T, C, Hh, Ww)
                right = to_nchw(rw).view(B, T, C, Hh, Ww)
        else:
            left, right = batch['left_eye_patch'], batch['right_eye_patch']
        if x_padded is None and left.dtype == torch.uint8:
            # decoded frames [B, T, H, W, C] (eve_sequences.py:196-203 not applied yet): normalise on the device --
            # straight into the stem's packed layout when the fused stem takes it, else to the reference's float NCHW
            from . import data
            B, T, Hh, Ww, C = left.shape
            if dt in HALF_DTYPES and C <= 4 and Hh % 4 == 0 and Ww == 128:
                x_padded = torch.empty((2 * B * T, Hh + 6, Ww + 8, 4), dtype=dt, device=left.device)
                k.frames_u8_to_stem(left.reshape(B * T, Hh, Ww, C), data.EYE_SCALE, data.EYE_SHIFT, out=x_padded[:B * T])
                k.frames_u8_to_stem(right.reshape(B * T, Hh, Ww, C), data.EYE_SCALE, data.EYE_SHIFT, out=x_padded[B * T:])
            else:
                left, right = data.preprocess_frames(left), data.preprocess_frames(right)
        if x_padded is None:
            B, T, C, Hh, Ww = left.shape
        cpad = pad_channels(C, dt)
        # float patches that require a gradient (a gaze loss for a generator, saliency, adversarial inputs) get it from the
        # stem's data-gradient kernel in every stem route; the default path below is unchanged when none does
        patches = None
        if _wants_grad(left) or _wants_grad(right):
            patches = (left.reshape(B * T, C, Hh, Ww), right.reshape(B * T, C, Hh, Ww))
            left, right = left.detach(), right.detach()         # (the packing launches below are outside the graph)
        if x_padded is not None:                                                   # packed from the uint8 frames above
            pass
        elif dt in HALF_DTYPES and C <= 4 and Hh % 4 == 0 and Ww == 128:        # fused stem: packed patches only
            x_padded = torch.empty((2 * B * T, Hh + 6, Ww + 8, 4), dtype=dt, device=left.device)
            k.stem_pack_input(left.reshape(B * T, C, Hh, Ww), out=x_padded[:B * T])
            k.stem_pack_input(right.reshape(B * T, C, Hh, Ww), out=x_padded[B * T:])
        else:
            stem_kernel = dt in HALF_DTYPES and C <= 4 and Hh % 4 == 0 and Ww % 128 == 0          # dedicated stem conv kernel
            # its weight gradient reads the packed patches too (ops.StemConvFn) while they stay below 2 GiB: the 8-channel NHWC
            # copy (2 GB at configs[4]'s 1 920 frames of 256 x 256) is then not made at all
            packed_wgrad = stem_kernel and 2 * B * T * (Hh + 6) * (Ww + 8) * 8 < (1 << 31)
            if not packed_wgrad:
                x = torch.empty((2 * B * T, Hh, Ww, cpad), dtype=dt, device=left.device)
                k.nchw_to_nhwc(left.reshape(B * T, C, Hh, Ww), dt, cpad, out=x[:B * T])
                k.nchw_to_nhwc(right.reshape(B * T, C, Hh, Ww), dt, cpad, out=x[B * T:])
            if stem_kernel:
                x_padded = torch.empty((2 * B * T, Hh + 6, Ww + 8, 4), dtype=dt, device=left.device)
                k.stem_pack_input(left.reshape(B * T, C, Hh, Ww), out=x_padded[:B * T])
                k.stem_pack_input(right.reshape(B * T, C, Hh, Ww), out=x_padded[B * T:])
        return self._trunk(x, P, x_padded, patches), B, T

    def _sequence_tail(self, feats, batch, B, T, initial_states, P):
        head_pose = None
        if self.config.eye_net_use_head_pose_input:
            head_pose = torch.cat([batch['left_h'].reshape(B * T, 2), batch['right_h'].reshape(B * T, 2)], dim=0)
        ncell = len(self.rnn_cells) if self.config.eye_net_use_rnn else 0
        h0 = None
        if initial_states is not None and ncell:
            def per_cell(v):                      # a bare tensor is the first cell's hidden state
                return list(v) if isinstance(v, (list,)) else [v] + [None] * (ncell - 1)
            lft, rgt = per_cell(initial_states['left']), per_cell(initial_states['right'])
            h0 = []
            for a, b in zip(lft, rgt):
                if a is None:
                    h0.append(None)
                elif isinstance(a, tuple):
                    h0.append(tuple(torch.cat([x_, y_], dim=0) for x_, y_ in zip(a, b)))
                else:
                    h0.append(torch.cat([a, b], dim=0))
        gaze, pupil, states = self._tail(feats, head_pose, 2 * B, T, h0, P)
        out = {}
        for si, side in enumerate(('left', 'right')):
            sl = slice(si * B * T, (si + 1) * B * T)
            g = gaze[sl].reshape(B, T, 2)
            out[side + '_g_initial'] = g.detach() if self.config.eye_net_frozen else g
            out[side + '_pupil_size'] = pupil[sl].reshape(B, T)
            for i in range(ncell):
                st = states[i]
                cut = slice(si * B, (si + 1) * B)
                out[side + '_eye_rnn_states_%d' % i] = tuple(s_[cut] for s_ in st) if isinstance(st, tuple) else st[cut]
        return out

    # ------------------------------------------------------------------ streaming (eve_amd/stream.py)
    # The shipped tail (one GRU cell, H = 128, head-pose input) can run as ONE eve_eye_tail_stream_fwd launch per chunk.  Off by
    # default: one workgroup per sequence streams the tail's 0.9 MB of weights through one CU, and that measured slower than the
    # layer-by-layer launches, which spread each layer over many CUs, at every shape tried (B x Tc = 1x1: 209 us for the kernel
    # against ~50 us for the 10 launches it replaces; whole steps 0.15-0.7 ms slower at 1x1 .. 32x30, profiles/stream_notes.md).
    stream_fused_tail = False

    def _stream_tail_fused_ok(self):
        cfg = self.config
        return (self.stream_fused_tail and cfg.eye_net_use_rnn and cfg.eye_net_rnn_type == 'GRU' and len(self.rnn_cells) == 1 and
                cfg.eye_net_use_head_pose_input and self.rnn_cells[0].hidden_size == 128 and
                self.fc_common[0].in_features == 130 and self.cnn_layers.fc.in_features == 512 and
                self.cnn_layers.fc.out_features == 128 and hasattr(default_kernels(), 'eye_tail_stream_fwd'))

    def _stream_state_buffers(self, B, device):
        """Zero-initialised carried states for B streams: per cell [2B, H] float32, the left eyes' rows then the right ones' (a
        pair (h, c) for LSTM) -- the layout `_tail` and the scans use.  STATIC EyeNet: none."""
        if not self.config.eye_net_use_rnn:
            return []
        z = lambda H: torch.zeros((2 * B, H), dtype=torch.float32, device=device)
        return [(z(c.hidden_size), z(c.hidden_size)) if self.config.eye_net_rnn_type == 'LSTM' else z(c.hidden_size)
                for c in self.rnn_cells]

    def _stream_tail_weights(self, P):
        """The 17 float32 tensors of include/eve_hip.h eve_eye_tail_weights, from the packs P (cached with them)."""
        cached = getattr(self, '_stream_w', None)
        if cached is not None and cached[0] is P:
            return cached[1]
        b = lambda t: t.detach().float().contiguous()
        cell = self.rnn_cells[0]
        w = (P['fc'].ihwo, b(self.cnn_layers.fc.bias), P['fc_common.0'].ihwo, b(self.fc_common[0].bias),
             P['fc_common.2'].ihwo, b(self.fc_common[2].bias), P['rnn.0.ih'].ihwo, b(cell.bias_ih), P['rnn.0.hh'].ihwo,
             b(cell.bias_hh), P['fc_to_gaze.0'].ihwo, b(self.fc_to_gaze[0].bias), P['fc_to_gaze.2'].ihwo,
             P['fc_to_pupil.0'].ihwo, b(self.fc_to_pupil[0].bias), P['fc_to_pupil.2'].ihwo, b(self.fc_to_pupil[2].bias))
        self._stream_w = (P, w)
        return w

    def _stream_sequence(self, batch, states, reset=None, lengths=None, plan=None):
        """One chunk of B streams (eval, no labels): batch as for forward_sequence ([B, Tc, ...]); states: the carried buffers of
        _stream_state_buffers, read as the state before the chunk's first frame -- zeroed first where reset[s] != 0 (int32 [2B], a
        stream's flag repeated for its two eyes) -- and overwritten with the state after its last frame.  `_tail` runs with the
        buffers as h0 and one eve_stream_state_rows launch per state each way; with stream_fused_tail the shipped tail is one
        eve_eye_tail_stream_fwd launch that reads and writes its state in place.  lengths: None, or int32 [2B] on the device laid
        out like reset -- sequence s then consumes only its first lengths[s] frames: its states are committed from frame
        lengths[s] - 1 (eve_stream_state_rows_at, eve_eye_tail_stream_fwd_len) or kept when that is 0, and its outputs from frame
        lengths[s] on are unspecified.  plan: None, or kernels.stream_mask_plan's result for this chunk (a masked step; it holds
        the lengths already) -- sequence s then consumes exactly its usable frames, in order: the trunk's features and the head
        pose are gathered through the plan's perm (usable frames first), the tail runs as in a ragged step with the usable
        counts as lengths, and gaze and pupil are gathered back through inv; entries at unusable eyes are unspecified.
        Returns the forward_sequence prediction keys (<side>_g_initial, <side>_pupil_size)."""
        k = default_kernels()
        batch = eye_pose_batch(batch, self.config, huber_px=self.face_huber_px)
        P = self._get_packs()
        feats, B, T = self._sequence_features(batch, P)
        head_pose = None
        if self.config.eye_net_use_head_pose_input:
            head_pose = torch.cat([batch['left_h'].reshape(B * T, 2), batch['right_h'].reshape(B * T, 2)], dim=0).float()
        if plan is not None:
            perm, lengths = plan['perm'][:2 * B], plan['count'][:2 * B]
            feats = k.stream_permute_rows(feats.view(2 * B, T, -1), perm).view(2 * B * T, -1)
            if head_pose is not None:
                head_pose = k.stream_permute_rows(head_pose.view(2 * B, T, 2), perm).view(2 * B * T, 2)
        if self._stream_tail_fused_ok():
            if lengths is None:
                gaze, pupil, _ = k.eye_tail_stream_fwd(feats, head_pose, self._stream_tail_weights(P), states[0], reset)
            else:
                gaze, pupil, _ = k.eye_tail_stream_fwd_len(feats, head_pose, self._stream_tail_weights(P), states[0], lengths, reset)
            gaze, pupil = gaze.view(2 * B * T, 2), pupil.view(2 * B * T)
        else:
            flat = [t for s_ in states for t in (s_ if isinstance(s_, tuple) else (s_,))]
            if reset is not None:
                for t in flat:
                    k.stream_state_rows(t, t, reset)
            gaze, pupil, out_states = self._tail(feats, head_pose, 2 * B, T, list(states) if states else None, P)
            for buf, st in zip(states, out_states or []):
                pairs = zip(buf, st) if isinstance(buf, tuple) else ((buf, st),)
                for dst, src in pairs:
                    if lengths is None:
                        k.stream_state_rows(src[:, -1], dst)
                    else:
                        k.stream_state_rows_at(src, dst, lengths)
        if plan is not None:
            back = plan['inv'][:2 * B]
            gaze = k.stream_permute_rows(gaze.view(2 * B, T, 2), back).view(2 * B * T, 2)
            pupil = k.stream_permute_rows(pupil.view(2 * B, T), back).view(2 * B * T)
        out = {}
        for si, side in enumerate(('left', 'right')):
            sl = slice(si * B * T, (si + 1) * B * T)
            out[side + '_g_initial'] = gaze[sl].reshape(B, T, 2)
            out[side + '_pupil_size'] = pupil[sl].reshape(B, T)
        return out
