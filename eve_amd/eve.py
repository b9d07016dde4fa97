"""EVE: the sequence harness around EyeNet and RefineNet -- drop-in for /root/reference/src/models/eve.py (class EVE).

Same constructor (`EVE(output_predictions=False)`, reads the config singleton), same call
(`model(full_input_dict, create_images=False, current_epoch=None)`; in training mode the argument is a dict holding
ONE data-source dict, eve.py:70-72), same result: a dict with `left/right_pupil_size`, every `loss_*` / `metric_*`
scalar of eve.py:286-439, the weighted `full_loss` (:234-265), the prediction tensors when `output_predictions`
(:194-222) and the visualisation maps when `create_images` (:268-283).  The input dict is extended in place with the
synthesised labels exactly as the reference does (:441-543).

What differs is the schedule.  The reference walks the clip frame by frame and runs ~60 small torch ops + Python-side
per-sample loops per frame; outside the two recurrent networks every frame (b, t) is independent, so here
  * EyeNet and RefineNet run over whole clips (`forward_sequence`: the recurrences are scans inside the modules),
  * gaze geometry (models/common.py:157-229), Gaussian heat-maps (:236-255) and soft-argmax (:304-333) are one HIP
    kernel each over the N = B*T frames (csrc/gaze_geometry.hip, autograd through ops.GazeToPoGFn / MakeHeatmapsFn /
    SoftArgmaxFn),
  * the O(T^2) gaze-history maps (:256-297) are built only for `create_images` (nothing else reads them),
  * the combined L/R gaze angles `g_*` (:136-154) feed metrics only and are returned without a graph.
The masked-loss reductions are device-side tensor ops on [B, T, ...] values (losses.py).
"""
import numpy as np
import torch
import torch.nn as nn

from . import losses, ops
from .config import get_config
from .eye_net import EyeNet, eye_input, eye_pose_batch, face_landmarks_key, has_pose_form
from .kernels import default_kernels
from .refine_net import screen_capture


def _mean2(a, b):
    return torch.stack([a, b], dim=-1).mean(dim=-1)


def _fuse2(a, b, eye_valid):
    """The binocular value of a masked EVEStream step, a, b [B, T, ...] for the left and the right eye, eye_valid bool [B, T, 2]:
    _mean2's bits where both eyes are usable, the usable eye's own value where one is (the right one's where none is: such a
    frame is invalid).  Selects only: whatever the other eye holds -- a NaN included -- does not reach the result."""
    left, right = (eye_valid[:, :, e].reshape(eye_valid.shape[:2] + (1,) * (a.dim() - 2)) for e in (0, 1))
    return torch.where(left & right, _mean2(a, b), torch.where(left, a, b))


def _u8(t):
    """A contiguous bool or uint8 tensor (or None) as the uint8 the launches read: a view, no copy."""
    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _f32(t, B, T, *tail):
    """t as [B, T] + tail, float32 and contiguous: what the stage launches read."""
    return t.reshape((B, T) + tail).float().contiguous()


class EVE(nn.Module):
    def __init__(self, output_predictions=False):
        super(EVE, self).__init__()
        config = get_config()
        self.config = config
        self.output_predictions = output_predictions
        if config.eye_net_load_pretrained or (config.refine_net_enabled and config.refine_net_load_pretrained):
            # utils/load_model.py downloads the released weights; there is no network on the hot path's side of the fence
            raise RuntimeError('eve_amd.EVE: *_load_pretrained needs the released checkpoints; load them with '
                               'load_state_dict (same keys as the reference) and set the config flag to False')
        self.eye_net = EyeNet()                                       # eve.py:55-60
        if config.eye_net_frozen:
            for p in self.eye_net.parameters():
                p.requires_grad = False
        self.refine_net = None
        if config.refine_net_enabled:                                 # eve.py:65
            from .refine_net import RefineNet
            self.refine_net = RefineNet()

    # ------------------------------------------------------------------------------------------ kappa draw (eve.py:463-479)
    @staticmethod
    def _draw_kappa(B, T, std):
        """The reference's draw: same amounts, same order, same global numpy RNG (:463-466), repeated over T (:467-479)."""
        draws = {'left': np.random.normal(size=(B, 2), loc=0.0, scale=std),
                 'right': np.random.normal(size=(B, 2), loc=0.0, scale=std)}
        return {side: np.repeat(np.expand_dims(draws[side], axis=1), T, axis=1).astype(np.float32) for side in draws}

    def refresh_static_kappa(self, B, T, device):
        """One host draw per optimiser step into FIXED device buffers (allocated on first use): what lets the whole train
        step be captured into a hipGraph although the reference draws kappa_fake on the host inside forward.  The sequence
        of draws is the eager path's: one call here per train.Trainer.step().
        The host never waits for the GPU under replay, so it may be several steps ahead: the draws go through a RING of
        pinned staging buffers, each guarded by the event of the copy that last read it -- a slot is rewritten only after
        its DMA has run (one pinned buffer per side was torn / reused by later draws).  The static buffers are used by
        calculate_additional_labels only while `_static_kappa_active` is set (Trainer sets it around capture / replay), so
        an eager step on the same model draws afresh."""
        cfg = self.config
        if not (self.training and cfg.refine_net_do_offset_augmentation):
            return
        std = np.radians(cfg.refine_net_offset_augmentation_sigma)
        static = getattr(self, '_static_kappa', None)
        if static is None or static['both'].shape[1:3] != (B, T) or static['both'].device != device:
            both = torch.empty((2, B, T, 2), dtype=torch.float32, device=device)
            static = {'both': both, 'left': both[0], 'right': both[1]}
            cuda = device.type == 'cuda'
            self._static_ring = [{'host': torch.empty((2, B, T, 2), dtype=torch.float32).pin_memory() if cuda
                                  else torch.empty((2, B, T, 2), dtype=torch.float32),
                                  'event': torch.cuda.Event() if cuda else None, 'used': False}
                                 for _ in range(self.STATIC_KAPPA_RING)]
            self._static_ring_pos = 0
            self._static_kappa = static
        slot = self._static_ring[self._static_ring_pos]
        self._static_ring_pos = (self._static_ring_pos + 1) % len(self._static_ring)
        if slot['used'] and slot['event'] is not None:
            slot['event'].synchronize()              # the copy that read this slot STATIC_KAPPA_RING steps ago has run
        kap = self._draw_kappa(B, T, std)
        slot['host'][0].copy_(torch.from_numpy(kap['left']))
        slot['host'][1].copy_(torch.from_numpy(kap['right']))
        static['both'].copy_(slot['host'], non_blocking=True)
        if slot['event'] is not None:
            slot['event'].record()
        slot['used'] = True

    STATIC_KAPPA_RING = 4
    _static_kappa_active = False

    def drop_static_kappa(self):
        self._static_kappa = None
        self._static_kappa_active = False

    # ------------------------------------------------------------------------------------------ labels (eve.py:441-543)
    def calculate_additional_labels(self, d, current_epoch=None):
        cfg = self.config
        sample = next(iter(d.values()))
        B, T = sample.shape[0], sample.shape[1]
        dev = sample.device
        k = default_kernels()
        for side in ('left', 'right'):
            if side + '_PoG_tobii' in d:
                d[side + '_PoG_cm_tobii'] = (d[side + '_PoG_tobii'] * (0.1 * d['millimeters_per_pixel'])).detach()
                d[side + '_PoG_cm_tobii_validity'] = d[side + '_PoG_tobii_validity']
        if self.training and cfg.refine_net_do_offset_augmentation:
            assert isinstance(current_epoch, float)
            std = np.radians(cfg.refine_net_offset_augmentation_sigma)
            static = getattr(self, '_static_kappa', None) if self._static_kappa_active else None
            if static is not None and tuple(static['left'].shape[:2]) == (B, T):
                # hipGraph replay (train.eve_trainer(use_graph=True)): the draw happened on the host BEFORE the replay
                # (refresh_static_kappa) and sits in fixed device buffers the captured kernels read; any other call (an
                # eager step on the same model, another batch shape) draws afresh below
                for side in ('left', 'right'):
                    d[side + '_kappa_fake'] = static[side]
            else:
                for side, kap in self._draw_kappa(B, T, std).items():
                    d[side + '_kappa_fake'] = torch.from_numpy(kap).to(dev)
        if 'left_o' in d:
            d['o'] = _mean2(d['left_o'], d['right_o']).detach()
            d['o_validity'] = d['left_o_validity']
        if 'left_PoG_tobii' in d:
            d['PoG_px_tobii'] = _mean2(d['left_PoG_tobii'], d['right_PoG_tobii']).detach()
            d['PoG_cm_tobii'] = _mean2(d['left_PoG_cm_tobii'], d['right_PoG_cm_tobii']).detach()
            valid = (d['left_PoG_tobii_validity'].bool() & d['right_PoG_tobii_validity'].bool()).detach()
            d['PoG_px_tobii_validity'] = d['PoG_cm_tobii_validity'] = valid
            if cfg.refine_net_enabled:
                w, h = cfg.gaze_heatmap_size
                centres = d['PoG_px_tobii'].reshape(B * T, 2).float()
                for name, sigma in (('initial', cfg.gaze_heatmap_sigma_initial), ('history', cfg.gaze_heatmap_sigma_history),
                                    ('final', cfg.gaze_heatmap_sigma_final)):
                    m = k.make_heatmaps(centres, sigma, (h, w), cfg.actual_screen_size, validity=valid.reshape(B * T))
                    d['heatmap_' + name] = m.view(B, T, 1, h, w)
                    d['heatmap_%s_validity' % name] = valid
        if 'PoG_cm_tobii' in d:
            d['g'] = k.combined_gaze(d['o'].reshape(B * T, 3), (10.0 * d['PoG_cm_tobii']).reshape(B * T, 2),
                                     d['left_R'].reshape(B * T, 3, 3), d['camera_transformation'].reshape(B * T, 4, 4)).view(B, T, 2)
            d['g_validity'] = d['PoG_cm_tobii_validity']

    # ------------------------------------------------------------------------------------------ eve.py:545-601
    def _pog_block(self, d, inter, g_key, out_suffix, kappa_suffix=None, heatmap_history=False, eye_valid=None, calib=None):
        """Per-eye PoG from `<side>_g_<g_key>`, their mean, the combined gaze, the heat-map -- for all B*T frames.  With
        `kappa_suffix` the offset augmentation is applied first and the augmented angles are stored back under
        `<side>_g_<kappa_suffix>`.  eye_valid (a masked EVEStream step: bool [B, T, 2]): the binocular PoG is the usable eye's own
        where only one is (_fuse2), and the combined gaze is rotated by d['combined_R'] (_predict_sequence).  calib (a calibrated
        EVEStream step): {'kappa': float32 [B, 2, 2] (stream, eye, (pitch, yaw)), 'calibrated': bool [B]} -- per eye a second
        eve_gaze_to_pog launch applies the stream's kappa row through the kernel's offset path, and a select per stream keeps the
        plain launch's bits where the stream is not calibrated (a zero row through the trigonometric round trip is not the
        identity in float32); `<side>_g_<g_key>` becomes the calibrated angles and the network's own stay under
        `<side>_g_<g_key>_raw`."""
        if 'inv_camera_transformation' not in d:                      # GazeCapture / MPIIGaze style inputs
            if kappa_suffix is not None:
                self._augment_only(d, inter, g_key, kappa_suffix)
            return
        cfg = self.config
        B, T = d['inv_camera_transformation'].shape[:2]
        N = B * T
        flat = lambda key, *s: d[key].reshape(N, *s).float()
        for side in ('left', 'right'):
            origin = inter[side + '_o'] if side + '_o' in inter else d[side + '_o']
            rot = inter[side + '_R'] if side + '_R' in inter else d[side + '_R']
            head_R = kappa = None
            if kappa_suffix is not None:
                head_R, kappa = flat('head_R', 3, 3), flat(side + '_kappa_fake', 2)
            g_out, mm, px = ops.GazeToPoGFn.apply(
                inter['%s_g_%s' % (side, g_key)].reshape(N, 2), origin.reshape(N, 3).float(), rot.reshape(N, 3, 3).float(),
                flat('inv_camera_transformation', 4, 4), flat('pixels_per_millimeter', 2), tuple(cfg.actual_screen_size),
                head_R, kappa)
            if kappa_suffix is not None:
                inter['%s_g_%s' % (side, kappa_suffix)] = g_out.view(B, T, 2)
            if calib is not None:
                g_raw = inter['%s_g_%s' % (side, g_key)]
                kap = calib['kappa'][:, 0 if side == 'left' else 1, None, :].expand(B, T, 2).reshape(N, 2).contiguous()
                g_c, mm_c, px_c = ops.GazeToPoGFn.apply(
                    g_raw.reshape(N, 2), origin.reshape(N, 3).float(), rot.reshape(N, 3, 3).float(),
                    flat('inv_camera_transformation', 4, 4), flat('pixels_per_millimeter', 2), tuple(cfg.actual_screen_size),
                    flat('head_R', 3, 3), kap)
                sel = calib['calibrated'][:, None, None]
                pick = lambda a, b: torch.where(sel, a.view(B, T, 2), b.view(B, T, 2))
                inter['%s_g_%s_raw' % (side, g_key)] = g_raw
                inter['%s_g_%s' % (side, g_key)] = pick(g_c, g_raw)
                mm, px = pick(mm_c, mm), pick(px_c, px)
            inter['%s_PoG_cm_%s' % (side, out_suffix)] = (0.1 * mm).view(B, T, 2)
            inter['%s_PoG_px_%s' % (side, out_suffix)] = px.view(B, T, 2)
        for unit in ('px', 'cm'):
            both = inter['left_PoG_%s_%s' % (unit, out_suffix)], inter['right_PoG_%s_%s' % (unit, out_suffix)]
            inter['PoG_%s_%s' % (unit, out_suffix)] = _mean2(*both) if eye_valid is None else _fuse2(both[0], both[1], eye_valid)
        inter['PoG_mm_' + out_suffix] = 10.0 * inter['PoG_cm_' + out_suffix]
        inter['g_' + out_suffix] = self._combined_gaze(d, inter['PoG_mm_' + out_suffix], B, T)
        if cfg.refine_net_enabled:
            w, h = cfg.gaze_heatmap_size
            centres = inter['PoG_px_' + out_suffix].reshape(N, 2)
            inter['heatmap_' + out_suffix] = ops.MakeHeatmapsFn.apply(
                centres, cfg.gaze_heatmap_sigma_initial, (h, w), tuple(cfg.actual_screen_size)).view(B, T, 1, h, w)
            if heatmap_history and 'PoG_px_tobii' in d:
                hist = default_kernels().make_heatmaps(centres.detach(), cfg.gaze_heatmap_sigma_history, (h, w),
                                                       tuple(cfg.actual_screen_size)).view(B, T, 1, h, w)
                inter['history_' + out_suffix] = self._history_maps(d['timestamps'], hist, d['PoG_px_tobii_validity'])

    def _augment_only(self, d, inter, g_key, kappa_suffix):
        """apply_offset_augmentation without camera geometry: the kernel's PoG outputs are computed against an identity
        camera and discarded (only head_R and kappa enter the augmented angles)."""
        B, T = d['head_R'].shape[:2]
        N = B * T
        dev = d['head_R'].device
        eye3 = torch.eye(3, device=dev).expand(N, 3, 3).contiguous()
        eye4 = torch.eye(4, device=dev).expand(N, 4, 4).contiguous()
        origin = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(N, 3).contiguous()
        for side in ('left', 'right'):
            g_out, _, _ = ops.GazeToPoGFn.apply(
                inter['%s_g_%s' % (side, g_key)].reshape(N, 2), origin, eye3, eye4, torch.ones((N, 2), device=dev),
                tuple(self.config.actual_screen_size), d['head_R'].reshape(N, 3, 3).float(),
                d[side + '_kappa_fake'].reshape(N, 2).float())
            inter['%s_g_%s' % (side, kappa_suffix)] = g_out.view(B, T, 2)

    def _history_maps(self, timestamps, heatmaps, validity):
        """common.py:256-297 for the full window: per clip, sum over frames with a non-zero timestamp of
        validity * decay^(ms before the clip's last non-zero timestamp) * heat-map.  Visualisation only."""
        ts = timestamps.to(torch.int64)
        nz = ts != 0
        idx = torch.arange(ts.shape[1], device=ts.device).expand_as(ts)
        last = torch.where(nz, idx, torch.full_like(idx, -1)).max(dim=1).values.clamp(min=0)
        target = ts.gather(1, last.view(-1, 1))
        diff_ms = ((target - ts) * 1e-6).float()
        wgt = torch.pow(torch.tensor(self.config.gaze_history_map_decay_per_ms, device=ts.device), diff_ms)
        wgt = wgt * nz.float() * validity.float()
        return (heatmaps * wgt.view(*wgt.shape, 1, 1, 1)).sum(dim=1)

    # ------------------------------------------------------------------------------------------ eve.py:69-284
    def forward(self, full_input_dict, create_images=False, current_epoch=None):
        cfg = self.config
        if self.training:
            assert len(full_input_dict) == 1
            full_input_dict = next(iter(full_input_dict.values()))
        # (the pose form -- camera_frame + eye_pose -- becomes the warp form in a copy, before the labels read left_o and left_R;
        # so does the face-landmark form, camera_frame + face_landmarks + face_rig: every sequence of a clip starts cold at t = 0)
        d = eye_pose_batch(full_input_dict, cfg, huber_px=self.eye_net.face_huber_px)
        self.calculate_additional_labels(d, current_epoch=current_epoch)
        B, T = eye_input(d).shape[:2]

        inter = dict(self.eye_net.forward_sequence(d))                # eve.py:105-111 for every t
        if self.training and cfg.refine_net_do_offset_augmentation:   # eve.py:114-135
            self._pog_block(d, inter, 'initial', 'initial_unaugmented')
            for side in ('left', 'right'):
                inter[side + '_g_initial_unaugmented'] = inter[side + '_g_initial']
            # augmented angles -> `<side>_g_initial`; the PoG block on them is both 'initial_augmented' and 'initial'
            self._pog_block(d, inter, 'initial_unaugmented', 'initial', kappa_suffix='initial', heatmap_history=create_images)
            for key in list(inter.keys()):
                if key.endswith('_initial') and ('PoG' in key or key in ('g_initial', 'heatmap_initial')):
                    inter[key + '_augmented'] = inter[key]
        else:
            self._pog_block(d, inter, 'initial', 'initial', heatmap_history=create_images)   # eve.py:138-143

        refined_history = None
        if self.refine_net is not None:                               # eve.py:146-166
            # (a BGR(A), NV12, I420 or YUYV capture goes in under its own key: reordered / converted inside the area resize)
            hf, states = self.refine_net.forward_sequence(inter['heatmap_initial'], d.get('screen_frame'), **screen_capture(d))
            inter['heatmap_final'] = hf
            for i, st in enumerate(states):
                if not isinstance(st, tuple):
                    inter['refinenet_rnn_states_%d' % i] = st
            self._final_block(d, inter, hf)
            if create_images and 'PoG_px_tobii' in d:
                refined_history = self._history_maps(d['timestamps'], hf.detach().float(), d['PoG_px_tobii_validity'])

        output_dict = {k_: v for k_, v in inter.items() if k_.startswith('output_')}
        output_dict['left_pupil_size'] = inter['left_pupil_size']
        output_dict['right_pupil_size'] = inter['right_pupil_size']
        if has_pose_form(full_input_dict):                            # the pose forms: reported, folded into no validity
            output_dict['pose_valid'] = d['pose_valid']
            if face_landmarks_key(full_input_dict) is not None:       # the head pose was solved here: the translation and the fit
                output_dict['head_t'], output_dict['face_reproj_rms'] = d['head_t'], d['face_reproj_rms']
                if 'face_inliers' in d:                               # (face_landmarks_raw or face_huber_px: eve_face_pose_solve_ex ran)
                    output_dict['face_inliers'] = d['face_inliers']
        if self.output_predictions:                                   # eve.py:194-222
            for key in ('timestamps', 'o', 'left_R', 'head_R', 'millimeters_per_pixel', 'pixels_per_millimeter',
                        'camera_transformation', 'inv_camera_transformation'):
                output_dict[key] = d[key]
            for key in ('g_initial', 'PoG_px_initial', 'PoG_cm_initial'):
                output_dict[key] = inter[key]
            if 'g' in d:
                output_dict['g'] = d['g']
                output_dict['validity'] = d['PoG_px_tobii_validity']
                output_dict['PoG_cm'] = d['PoG_cm_tobii']
                output_dict['PoG_px'] = d['PoG_px_tobii']
            if self.refine_net is not None:
                for key in ('g_final', 'PoG_px_final', 'PoG_cm_final'):
                    output_dict[key] = inter[key]

        self.calculate_losses_and_metrics(d, inter, output_dict)
        output_dict['full_loss'] = self._full_loss(output_dict, eye_input(d).device)

        if create_images:                                             # eve.py:268-283
            if cfg.load_screen_content:
                if 'screen_frame' in d:                               # (a screen_frame_bgr / _nv12 / _i420 / _yuyv capture is not echoed)
                    output_dict['screen_frame'] = d['screen_frame'][:, -1]
            if 'history_initial' in inter:
                output_dict['initial_gaze_history'] = inter['history_initial']
            if 'heatmap_initial' in inter:
                output_dict['initial_heatmap'] = inter['heatmap_initial'][:, -1]
            if 'heatmap_final' in inter:
                output_dict['final_heatmap'] = inter['heatmap_final'][:, -1]
                output_dict['refined_gaze_history'] = refined_history
            if 'heatmap_final' in d:
                output_dict['gt_heatmap'] = d['heatmap_final'][:, -1]
        return output_dict

    def _final_block(self, d, inter, hf):
        """eve.py:155-166: the refined PoG by soft-argmax of heatmap_final [B, T, 1, h, w], in px and cm, and the combined gaze
        (rotated by d['combined_R'] where a masked EVEStream step has put one, by left_R as in the reference otherwise)."""
        cfg = self.config
        B, T = hf.shape[:2]
        h, w = hf.shape[-2:]
        px = ops.SoftArgmaxFn.apply(hf.reshape(B * T, 1, h, w).float(), tuple(cfg.actual_screen_size)).view(B, T, 2)
        inter['PoG_px_final'] = px
        inter['PoG_cm_final'] = self._px_to_cm(d, px)
        inter['g_final'] = self._combined_gaze(d, 10.0 * inter['PoG_cm_final'], B, T)

    @staticmethod
    def _px_to_cm(d, px):
        """A point in screen pixels [B, T, 2] -> centimetres (eve.py:160)."""
        return px * (0.1 * d['millimeters_per_pixel'])

    @staticmethod
    def _combined_gaze(d, pog_mm, B, T):
        """The combined gaze angles [B, T, 2] towards a point in millimetres on the screen, from the binocular origin d['o'], rotated
        by d['combined_R'] where a masked EVEStream step has put one, by left_R as in the reference otherwise."""
        return default_kernels().combined_gaze(
            d['o'].reshape(B * T, 3).float(), pog_mm.detach().reshape(B * T, 2),
            d.get('combined_R', d['left_R']).reshape(B * T, 3, 3).float(), d['camera_transformation'].reshape(B * T, 4, 4).float()).view(B, T, 2)

    # ------------------------------------------------------------------------------------------ streaming (stream.py)
    PREDICTION_KEYS = ('left_g_initial', 'right_g_initial', 'left_pupil_size', 'right_pupil_size', 'g_initial', 'PoG_px_initial',
                       'PoG_cm_initial', 'g_final', 'PoG_px_final', 'PoG_cm_final')

    def _predict_sequence(self, d, eye_states, refine_states, reset=None, return_heatmaps=False, lengths=None, masked=False,
                          eye_mask=None, pose_gate=None, face_state=None, render=None, calibration=None, events=None, gate=None,
                          screen_calibration=None, history=None, aoi=None, pupil=None, luminance=None, saccades=None,
                          pursuits=None):
        """The prediction part of forward() for one chunk of an EVEStream: eval only, no labels, no losses.  d: the chunk's
        inputs [B, Tc, ...] (not modified; camera_frame may be any one key of eye_net.EYE_FRAME_KEYS or camera_surface, and the screen any one
        key of refine_net.SCREEN_FRAME_KEYS or screen_surface; the eyes as patches, as camera_frame + {left,right}_eye_warp, or as camera_frame +
        eye_pose [B, Tc, 18], which also stands in for {left,right}_h / _o / _R and head_R and adds pose_valid to the result; both
        camera forms with an optional camera_lens [B, Tc, 12] for raw frames -- eye_net.eye_input, eye_pose_batch); eye_states / refine_states: the carried state buffers of the two networks
        (EyeNet._stream_state_buffers, RefineNet._stream_state_buffers), read as the state before the chunk and overwritten with
        the state after it; reset: None or int32 [2B] device flags (stream b's flag at b and B + b) -- flagged streams start from
        zero; lengths: None or int32 [2B] device frame counts in the same layout -- stream b consumes its first lengths[b] frames
        only (states handed over from frame lengths[b] - 1, outputs from lengths[b] on unspecified).  Same kernels and the same
        _pog_block / _final_block as forward().  -> the PREDICTION_KEYS present (the PoG keys need the camera geometry), plus
        heatmap_final when asked.
        masked (EVEStream.step(eye_mask=..., skip_invalid_pose=...)): eye_mask None or uint8 / bool [B, Tc, 2] on the device
        (left, right; non-zero = usable); pose_gate None, or with the pose form a bool [1] device tensor -- pose_valid is ANDed
        into the mask where it holds False (a device value, so one captured graph serves both settings).  One
        eve_stream_mask_plan launch turns mask, pose_valid and lengths into the plan both networks compact their sequences by
        (EyeNet._stream_sequence, RefineNet._stream_sequence); the binocular quantities come from the usable eyes by selects:
        PoG_*_initial and o through _fuse2 (both usable: the mean's bits), and the combined gaze g_initial / g_final is rotated by
        left_R where the left eye is usable, else by right_R -- an approximation the reference never needed (it always has
        both eyes and rotates by left_R).  The result gains valid [B, Tc] and eye_valid [B, Tc, 2], bool.
        face_state: with the face-landmark form (camera_frame + face_landmarks [B, Tc, L, 2 | 3] + face_rig [B, 12 + 3L]) the
        stream's carried head pose, float64 [B, 13], read as the pose before the chunk and overwritten with the pose after it by
        the eve_face_pose_solve launch, which also reads reset[:B] and lengths[:B]; the result gains pose_valid, head_t and
        face_reproj_rms.  face_landmarks_raw (raw-frame pixels, with camera_lens) in place of face_landmarks, or
        eye_net.face_huber_px, make it the eve_face_pose_solve_ex launch, and the result gains face_inliers [B, Tc].
        render: None, or EVEStream's overlay hook render(d, inter, out), called last with the chunk after eye_pose_batch (the derived
        warps included), the intermediate results (heatmap_final whether returned or not) and the result, to which it adds
        `rendered`; None issues no launch.
        calibration: None, or EVEStream's per-person calibration {'kappa': float32 [B, 2, 2], 'ok': uint8 [B, 2], 'apply': bool,
        'store': None or (samples float64 [B, 2, C, 16], count int32 [B, 2], dropped int32 [B, 2])}.  With a store and
        calibration_target [B, Tc, 2] (and optionally calibration_valid [B, Tc]) in d, one eve_calib_append launch reduces every
        usable (frame, eye) -- calibration_valid, t < lengths[b], eye_valid -- from the network's own angles and appends it.  With
        apply, _pog_block applies the kappa rows where both flags of a stream are set; the result gains <side>_g_initial_raw and
        calibrated, bool [B].  None issues no launch.
        events: None, or EVEStream's gaze filter and fixation / saccade stage {'spec': a data.GazeEventSpec, 'source': the result key
        it filters, 'state': float64 [B, 32], 'store': float64 [B, F, 8], 'count', 'dropped': int32 [B]}: one eve_gaze_events launch,
        last before the render hook, over the step's own source PoG and d['o'], with frame_time from d when it is there, the step's
        lengths, `valid` (masked) and reset flags; the result gains data.GAZE_EVENT_KEYS.  None issues no launch.
        gate: None, or EVEStream's eye gate {'spec': a data.EyeGateSpec, 'state': float64 [B, 2, 8], 'store': float64 [B, capacity, 4],
        'count', 'dropped': int32 [B], 'frame_size': None or the camera frame's (IW, IH)}: one eve_eye_gate launch between eye_pose_batch and
        the mask plan, over pose_valid, face_reproj_rms, face_inliers, the (derived) warps and head angles and d['eye_contours'] -- each
        where the spec has a criterion for it -- with the step's lengths and reset flags.  Its `usable` becomes eye_mask, or is ANDed
        into it, so a gated step is a masked step; the result gains data.EYE_GATE_KEYS.  None issues no launch.
        screen_calibration: None, or EVEStream's screen-space map {'coef': float64 [B, 2, 6], 'kind': uint8 [B], 'apply': bool, 'store':
        None or (samples float64 [B, C, 12], count int32 [B], dropped int32 [B])}, a stage on the step's OUTPUT point PoG_px_<out>
        (<out> = final with a RefineNet, else initial) that runs before the events stage and the render hook.  With a store and
        screen_calibration_target [B, Tc, 2] (and optionally screen_calibration_valid [B, Tc]) in d, one eve_screen_calib_append launch
        appends every usable frame -- screen_calibration_valid, t < lengths[b], the masked plan's valid -- from the UNCORRECTED point.
        With apply, one eve_screen_calib_apply launch corrects the point: PoG_px_<out> becomes the corrected one, PoG_cm_<out> and
        g_<out> follow by _px_to_cm / _combined_gaze (selected per stream, so a stream of kind 0 keeps its bits), and the result gains
        PoG_px_<out>_raw and screen_calibrated, bool [B].  None issues no launch.
        history: None, or EVEStream's gaze history stage, a list of {'spec': a data.GazeHistorySpec, 'source': the result key it
        accumulates, 'P': the launches' scalars, 'state': float64 [B, 8], 'maps': float32 [B, MH, MW]}: per entry one
        eve_gaze_history_plan and one eve_gaze_history_update launch, after the events stage and before the render hook, over the step's
        own source (a point of gaze, or heatmap_final), with frame_time from d when it is there, the step's lengths, `valid` (masked)
        and reset flags; the result gains <name> (a copy of the carried map) and with per_frame <name>_frames.  None issues no launch.
        aoi: None, or EVEStream's areas-of-interest stage {'spec': a data.AoiSpec, 'source': the result key whose point is tested,
        'use_fixations': bool, 'state': float64 [B, 16], 'table': float64 [B, A + 1, 8], 'trans': int32 [B, A + 1, A], 'visits': float64
        [B, V, 8], 'count', 'dropped': int32 [B]}: one eve_gaze_aoi launch, after the history stage and before the render hook, over the
        step's own source point and d['aoi_shapes'] ([B, A, 36] or [B, Tc, A, 36]), with frame_time from d when it is there, the step's
        lengths, `valid` (masked) and reset flags, and with use_fixations the events stage's fixation_id / fixating; the result gains
        <name>_id, <name>_mask and <name>_visit_ms.  None issues no launch.
        pupil: None, or EVEStream's pupillometry stage {'spec': a data.PupilSpec, 'state': float64 [B, 32], 'table': float64 [B, 24],
        'light': float64 [B, 4], 'store': float64 [B, capacity, 8], 'count', 'dropped': int32 [B]}: one eve_pupil_track launch, after the
        AOI stage and before the render hook, over the step's own <side>_pupil_size, the mask plan's eye_valid (a masked or gated
        step), frame_time, pupil_luminance and pupil_baseline from d where they are there, the step's lengths and reset flags; the
        result gains <name>_<key> for data.PUPIL_KEYS.  None issues no launch.
        luminance: None, or EVEStream's screen-luminance stage {'spec': a data.ScreenLuminanceSpec, 'key': the capture's chunk key,
        'layout': its data.SurfaceLayout, 'matrix', 'source': the result key the discs follow or None, 'radii': capture pixels, 'sx',
        'sy', 'table': the response table on the device}: one eve_screen_luminance launch, after the AOI stage and before the pupil
        stage, over the capture where it lies in d, the step's lengths and, for the discs, the masked plan's valid ANDed with the
        spec's valid_key; the result gains the spec's result_keys(), and with to_pupil and pupil= the covariate is the pupil stage's
        luminance.  None issues no launch.
        saccades: None, or EVEStream's saccade stage {'spec': a data.SaccadeSpec, 'state': float64 [B, 32], 'table': float64 [B, 16],
        'store': float64 [B, S, 16], 'count', 'dropped': int32 [B]}, which needs events: the events launch is then eve_gaze_events_ex,
        and one eve_gaze_saccades launch follows it, before the history stage, over that launch's sample flags, times and gaze vectors
        (which stay internal), its labels, velocities and fixation ids and the point the velocity is from, with the step's lengths and
        reset flags; the result gains saccade_id and saccade_ms.  None issues the launches a step without it issues.
        pursuits: None, or EVEStream's smooth-pursuit stage {'spec': a data.PursuitSpec, 'state': float64 [B, 320], 'table': float64
        [B, 16], 'store': float64 [B, S, 20], 'count', 'dropped': int32 [B]}, which needs events: the events launch is then
        eve_gaze_events_ex, and one eve_gaze_pursuits launch follows it (and the saccade launch, where there is one), before the
        history stage, over the same inputs plus the chunk's optional pursuit_target float32 [B, Tc, 2]; the result gains
        data.PURSUIT_KEYS.  None issues the launches a step without it issues."""
        assert not self.training, 'EVE._predict_sequence is eval-only'
        B = eye_input(d).shape[0]
        posed, faced = has_pose_form(d), face_landmarks_key(d) is not None
        contours = d.get('eye_contours')
        # reset and lengths hold a row per eye sequence [2B]; what works per stream reads the first B
        reset_b, lengths_b = None if reset is None else reset[:B], None if lengths is None else lengths[:B]
        d = dict(eye_pose_batch(d, self.config, face_state, reset_b, lengths_b, huber_px=self.eye_net.face_huber_px))
        plan = eye_valid = gated = None
        if gate is not None:
            gated = self._eye_gate(d, contours, gate, reset_b, lengths_b)
            eye_mask = gated['usable'] if eye_mask is None else (eye_mask != 0) & (gated['usable'] != 0)
            masked = True
        if masked:
            T = eye_input(d).shape[1]
            pose_ok = None
            if pose_gate is not None:
                pose_ok = (d['pose_valid'] | pose_gate).contiguous()
            plan = default_kernels().stream_mask_plan(B, T, eye_mask, pose_ok, lengths, device=eye_input(d).device)
            eye_valid = plan['eye_valid'].view(torch.bool)
        if 'left_o' in d:
            d['o'] = _mean2(d['left_o'], d['right_o']) if plan is None else _fuse2(d['left_o'], d['right_o'], eye_valid)
        if plan is not None and 'left_R' in d:
            d['combined_R'] = torch.where(eye_valid[:, :, 0, None, None], d['left_R'], d['right_R'])
        inter = dict(self.eye_net._stream_sequence(d, eye_states, reset, lengths, plan))
        calib = None
        if calibration is not None:
            if calibration['store'] is not None and 'calibration_target' in d:
                self._calibration_append(d, inter, calibration['store'], lengths_b, plan)
            if calibration['apply']:
                calib = {'kappa': calibration['kappa'], 'calibrated': (calibration['ok'] != 0).all(dim=1)}
        if calib is None:
            self._pog_block(d, inter, 'initial', 'initial', eye_valid=eye_valid)
        else:
            self._pog_block(d, inter, 'initial', 'initial', eye_valid=eye_valid, calib=calib)
        if self.refine_net is not None and 'heatmap_initial' in inter:
            hf = self.refine_net._stream_sequence(inter['heatmap_initial'], d.get('screen_frame'), refine_states, reset_b, lengths_b, plan,
                                                  **screen_capture(d))
            inter['heatmap_final'] = hf
            self._final_block(d, inter, hf)
        if screen_calibration is not None:
            self._screen_calibration(d, inter, screen_calibration, lengths_b, plan)
        out = {k_: inter[k_] for k_ in self.PREDICTION_KEYS if k_ in inter}
        if screen_calibration is not None and screen_calibration['apply']:
            suffix = 'final' if 'PoG_px_final' in inter else 'initial'
            out['PoG_px_%s_raw' % suffix] = inter['PoG_px_%s_raw' % suffix]
            out['screen_calibrated'] = inter['screen_calibrated']
        if calib is not None:
            out['calibrated'] = calib['calibrated']
            for side in ('left', 'right'):
                if side + '_g_initial_raw' in inter:
                    out[side + '_g_initial_raw'] = inter[side + '_g_initial_raw']
        if posed:
            out['pose_valid'] = d['pose_valid']
        if faced:
            out['head_t'], out['face_reproj_rms'] = d['head_t'], d['face_reproj_rms']
            if 'face_inliers' in d:
                out['face_inliers'] = d['face_inliers']
        if plan is not None:
            out['valid'], out['eye_valid'] = plan['valid'].view(torch.bool), eye_valid
        if gated is not None:
            out['eye_gate_reason'], out['eye_openness'], out['blink'] = gated['reason'], gated['openness'], gated['blink']
        if return_heatmaps and 'heatmap_final' in inter:
            out['heatmap_final'] = inter['heatmap_final']
        if events is not None:
            T = eye_input(d).shape[1]
            k = default_kernels()
            pog = _f32(inter[events['source']], B, T, 2)
            res = (k.gaze_events if saccades is None and pursuits is None else k.gaze_events_ex)(
                pog, _f32(d['o'], B, T, 3), _f32(d['inv_camera_transformation'], B, T, 4, 4),
                _f32(d['pixels_per_millimeter'], B, T, 2), events['spec'], events['state'], events['store'], events['count'], events['dropped'],
                frame_time=d['frame_time'].contiguous() if 'frame_time' in d else None, valid=None if plan is None else plan['valid'],
                lengths=lengths_b, reset=reset_b)
            if saccades is None and pursuits is None:
                out.update(res)
            else:
                from .data import GAZE_EVENT_KEYS, pursuit_stage, saccade_stage
                out.update({k_: res[k_] for k_ in GAZE_EVENT_KEYS})
                carried = lambda stage: [stage[k_] for k_ in ('state', 'table', 'store', 'count', 'dropped')]
                if saccades is not None:
                    out.update(saccade_stage(k, pog, res, events['spec'], saccades['spec'], carried(saccades), lengths=lengths_b, reset=reset_b))
                if pursuits is not None:
                    target = _f32(d['pursuit_target'], B, T, 2) if 'pursuit_target' in d else None
                    out.update(pursuit_stage(k, pog, res, events['spec'], pursuits['spec'], carried(pursuits), target=target, lengths=lengths_b,
                                             reset=reset_b))
        if history is not None:
            self._gaze_history(d, inter, out, history, lengths_b, reset_b, plan)
        if aoi is not None:
            self._gaze_aoi(d, inter, out, aoi, lengths_b, reset_b, plan)
        covariate = None
        if luminance is not None:
            covariate = self._screen_luminance(d, inter, out, luminance, lengths_b, plan)
        if pupil is not None and covariate is not None:
            self._pupil_track(d, inter, out, pupil, lengths_b, reset_b, plan, luminance=covariate)
        elif pupil is not None:
            self._pupil_track(d, inter, out, pupil, lengths_b, reset_b, plan)
        if render is not None:
            render(d, inter, out)
        return out

    def _gaze_history(self, d, inter, out, history, lengths, reset, plan):
        """The gaze history stage of an EVEStream step: per spec the time chain's launch (eve_gaze_history_plan) and the maps' launch
        (eve_gaze_history_update) on the carried buffers."""
        B, T = eye_input(d).shape[:2]
        k = default_kernels()
        screen = tuple(self.config.actual_screen_size)

        def look(key):
            for src in (out, inter, d):
                if key in src:
                    return src[key]
            raise ValueError('step: history: %r is neither in the chunk nor a result of this step' % (key,))

        frame_time = d['frame_time'].contiguous() if 'frame_time' in d else None
        for h in history:
            spec, P = h['spec'], h['P']
            valid_key = None if spec.valid_key is None else _u8(look(spec.valid_key).reshape(B, T))
            pog = heat = None
            if h['source'] == 'heatmap_final':
                heat = _f32(inter['heatmap_final'], B, T, *inter['heatmap_final'].shape[-2:])
            else:
                pog = _f32(look(h['source']), B, T, 2)
            coef, clear = k.gaze_history_plan(P, screen, h['state'], T, pog=pog, frame_time=frame_time,
                                              valid=None if plan is None else plan['valid'], valid_key=valid_key, lengths=lengths, reset=reset)
            frames = k.gaze_history_update(P, coef, clear, h['maps'], heat=heat, per_frame=spec.per_frame)
            out[spec.name] = h['maps'].clone()
            if spec.per_frame:
                out[spec.name + '_frames'] = frames

    def _gaze_aoi(self, d, inter, out, aoi, lengths, reset, plan):
        """The areas-of-interest stage of an EVEStream step: one eve_gaze_aoi launch on the carried buffers."""
        B, T = eye_input(d).shape[:2]
        spec = aoi['spec']

        def look(key):
            for src in (out, inter, d):
                if key in src:
                    return src[key]
            raise ValueError('step: aoi: %r is neither in the chunk nor a result of this step' % (key,))

        fix = {}
        if aoi['use_fixations']:
            fix = {'fixation_id': out['fixation_id'].contiguous(), 'fixating': _u8(out['fixating'].reshape(B, T))}
        res = default_kernels().gaze_aoi(
            _f32(look(aoi['source']), B, T, 2), d['aoi_shapes'].contiguous(), spec, aoi['state'], aoi['table'], aoi['trans'], aoi['visits'],
            aoi['count'], aoi['dropped'], frame_time=d['frame_time'].contiguous() if 'frame_time' in d else None,
            valid=None if plan is None else plan['valid'], valid_key=None if spec.valid_key is None else _u8(look(spec.valid_key).reshape(B, T)),
            lengths=lengths, reset=reset, **fix)
        for k_, v in res.items():
            out['%s_%s' % (spec.name, k_)] = v

    def _screen_luminance(self, d, inter, out, lum, lengths, plan):
        """The screen-luminance stage of an EVEStream step: one eve_screen_luminance launch on the capture where it lies (the chunk
        tensor; under a graph, its input buffer) -> the covariate float32 [B, T], or None without to_pupil."""
        from .data import luminance_results
        B, T = eye_input(d).shape[:2]
        spec = lum['spec']

        def look(key):
            for src in (out, inter, d):
                if key in src:
                    return src[key]
            raise ValueError('step: luminance: %r is neither in the chunk nor a result of this step' % (key,))

        centres = valid = None
        if spec.radii_px:
            centres = _f32(look(lum['source']), B, T, 2).reshape(B * T, 2)
            if plan is not None:
                valid = plan['valid'].reshape(B, T) != 0
            if spec.valid_key is not None:
                vk = look(spec.valid_key).reshape(B, T) != 0
                valid = vk if valid is None else valid & vk
            if valid is not None:
                valid = valid.to(torch.uint8).reshape(B * T).contiguous()
        frames = d[lum['key']]
        _, _, mean = default_kernels().screen_luminance(
            frames.reshape(B * T, -1), lum['layout'], lum['table'], spec.weights, B, T, radii=lum['radii'], centres=centres, sx=lum['sx'],
            sy=lum['sy'], centre_valid=valid, lengths=lengths, matrix=lum['matrix'])
        res = luminance_results(spec, mean, B, T)
        out.update(res)
        return res.get(spec.name + '_covariate')

    def _pupil_track(self, d, inter, out, pupil, lengths, reset, plan, luminance=None):
        """The pupillometry stage of an EVEStream step: one eve_pupil_track launch on the carried buffers.  luminance: None, or the
        screen-luminance stage's covariate of this step, in place of the chunk's pupil_luminance (the step refuses both)."""
        B, T = eye_input(d).shape[:2]
        spec = pupil['spec']
        size = torch.stack([_f32(inter['left_pupil_size'], B, T), _f32(inter['right_pupil_size'], B, T)])
        res = default_kernels().pupil_track(
            size, spec, pupil['state'], pupil['table'], pupil['light'], pupil['store'], pupil['count'], pupil['dropped'],
            eye_valid=None if plan is None else plan['eye_valid'], frame_time=d['frame_time'].contiguous() if 'frame_time' in d else None,
            lengths=lengths, reset=reset,
            luminance=luminance.contiguous() if luminance is not None else d['pupil_luminance'].contiguous() if 'pupil_luminance' in d else None,
            baseline_mark=_u8(d.get('pupil_baseline')))
        for k_, v in res.items():
            out['%s_%s' % (spec.name, k_)] = v

    def _eye_gate(self, d, contours, gate, reset, lengths):
        """The gate of a gated EVEStream step: one eve_eye_gate launch over what the spec has a criterion for (d: the chunk after
        eye_pose_batch, so the derived warps and head angles are there)."""
        from .data import eye_patch_hw
        spec = gate['spec']
        B, T = eye_input(d).shape[:2]
        both = lambda key, n: torch.stack([d['left' + key], d['right' + key]]).reshape(2, B * T, n).float().contiguous()
        ph, pw = eye_patch_hw(self.config)
        return default_kernels().eye_gate(
            spec, B, T, gate['state'], gate['store'], gate['count'], gate['dropped'], pose_valid=_u8(d.get('pose_valid')),
            reproj_rms=d['face_reproj_rms'].contiguous() if spec.max_reproj_px is not None else None,
            inliers=d['face_inliers'].contiguous() if spec.min_inliers is not None else None,
            warp=both('_eye_warp', 9) if spec.min_coverage is not None else None, h=both('_h', 2) if spec.head_angles else None,
            contours=contours.contiguous() if spec.blink is not None else None, lengths=lengths, reset=reset,
            frame_size=gate['frame_size'], patch_size=(pw, ph))

    def _calibration_append(self, d, inter, store, lengths, plan):
        """The collecting stage of a calibrated EVEStream step: one eve_calib_append launch over both eyes, from the network's own
        <side>_g_initial (before any calibration is applied, so collecting while calibrated does not compound)."""
        B, T = d['calibration_target'].shape[:2]
        both = lambda key, *s_: torch.stack([(inter[side + key] if side + key in inter else d[side + key]).reshape((B, T) + s_).float()
                                             for side in ('left', 'right')]).contiguous()
        default_kernels().calib_append(both('_g_initial', 2), _f32(d['head_R'], B, T, 3, 3), both('_o', 3), both('_R', 3, 3),
                                       _f32(d['inv_camera_transformation'], B, T, 4, 4), _f32(d['pixels_per_millimeter'], B, T, 2),
                                       _f32(d['calibration_target'], B, T, 2), store[0], store[1], store[2], _u8(d.get('calibration_valid')),
                                       lengths, None if plan is None else plan['eye_valid'])

    def _screen_calibration(self, d, inter, sc, lengths, plan):
        """The screen-space map's stage of an EVEStream step, on the output point PoG_px_<out>: the collecting launch
        (eve_screen_calib_append, on the uncorrected point, so collecting while the map is applied does not compound), then the
        applying one (eve_screen_calib_apply), after which PoG_cm_<out> and g_<out> are the expressions of _final_block on the
        corrected point where the stream has a map."""
        suffix = 'final' if 'PoG_px_final' in inter else 'initial'
        raw = inter['PoG_px_' + suffix]
        B, T = raw.shape[:2]
        size = tuple(self.config.actual_screen_size)
        ppm = _f32(d['pixels_per_millimeter'], B, T, 2)
        if sc['store'] is not None and 'screen_calibration_target' in d:
            default_kernels().screen_calib_append(_f32(raw, B, T, 2), _f32(d['o'], B, T, 3), _f32(d['inv_camera_transformation'], B, T, 4, 4), ppm,
                                                  _f32(d['screen_calibration_target'], B, T, 2), size, sc['store'][0], sc['store'][1],
                                                  sc['store'][2], _u8(d.get('screen_calibration_valid')), lengths,
                                                  None if plan is None else plan['valid'])
        if sc['apply']:
            px = default_kernels().screen_calib_apply(_f32(raw, B, T, 2), ppm, sc['coef'], sc['kind'], size).view(B, T, 2)
            mapped = sc['kind'] != 0
            sel = mapped[:, None, None]
            cm = self._px_to_cm(d, px)
            inter['PoG_px_%s_raw' % suffix] = raw
            inter['PoG_px_' + suffix] = px
            inter['PoG_cm_' + suffix] = torch.where(sel, cm, inter['PoG_cm_' + suffix])
            inter['g_' + suffix] = torch.where(sel, self._combined_gaze(d, 10.0 * cm, B, T), inter['g_' + suffix])
            inter['screen_calibrated'] = mapped

    # ------------------------------------------------------------------------------------------ eve.py:286-439
    def calculate_losses_and_metrics(self, d, inter, out):
        cfg = self.config
        augment = self.training and cfg.refine_net_do_offset_augmentation
        un = '_unaugmented' if augment else ''

        # the [B, T, D <= 3] terms are collected and evaluated by ONE kernel launch (ops.VectorTermsFn); heat-map terms, CPU
        # tensors and Euclidean terms that would need a gradient keep their own path
        batched = []
        kinds = {losses.mse_loss: 'mse', losses.euclidean_loss: 'euclidean', losses.l1_loss: 'l1', losses.angular_loss: 'angular'}

        def term(name, fn, interm_key, input_key, ref=None):
            ref = d if ref is None else ref
            if interm_key in inter and input_key in ref:
                pred, tgt, val = inter[interm_key], ref[input_key], ref[input_key + '_validity']
                kind = kinds.get(fn)
                if (kind is not None and pred.is_cuda and pred.dim() <= 3 and pred.dtype == torch.float32 and
                        tgt.dtype == torch.float32 and tuple(tgt.shape) == tuple(pred.shape) and not tgt.requires_grad and
                        (pred.dim() == 2 or pred.shape[2] <= 3) and not (kind == 'euclidean' and pred.requires_grad and
                                                                          torch.is_grad_enabled()) and
                        hasattr(default_kernels(), 'vector_terms')):
                    out[name] = None                         # (keeps the reference's key order)
                    batched.append((name, kind, pred, tgt, val))
                else:
                    out[name] = fn(pred, tgt, val)

        for side in ('left', 'right'):
            term('loss_ang_%s_g_initial' % side, losses.angular_loss, '%s_g_initial%s' % (side, un), side + '_g_tobii')
            term('loss_mse_%s_PoG_cm_initial' % side, losses.mse_loss, '%s_PoG_cm_initial%s' % (side, un), side + '_PoG_cm_tobii')
            term('metric_euc_%s_PoG_cm_initial' % side, losses.euclidean_loss, '%s_PoG_cm_initial%s' % (side, un), side + '_PoG_cm_tobii')
            term('metric_euc_%s_PoG_px_initial' % side, losses.euclidean_loss, side + '_PoG_px_initial', side + '_PoG_tobii')
            term('loss_l1_%s_pupil_size' % side, losses.l1_loss, side + '_pupil_size', side + '_p')
        if 'left_PoG_tobii' in d and 'right_PoG_tobii' in d:         # left-right consistency
            inter['right_PoG_cm_initial_validity'] = d['left_PoG_tobii_validity'] & d['right_PoG_tobii_validity']
            term('loss_mse_lr_consistency', losses.mse_loss, 'left_PoG_cm_initial', 'right_PoG_cm_initial', inter)
            term('metric_euc_lr_consistency', losses.euclidean_loss, 'left_PoG_cm_initial', 'right_PoG_cm_initial', inter)
        term('loss_ce_heatmap_initial', losses.bce_loss, 'heatmap_initial' + un, 'heatmap_initial')
        term('loss_ce_heatmap_final', losses.bce_loss, 'heatmap_final', 'heatmap_final')
        term('loss_mse_heatmap_final', losses.mse_loss, 'heatmap_final', 'heatmap_final')
        if cfg.refine_net_do_offset_augmentation:
            term('metric_euc_PoG_px_initial_unaugmented', losses.euclidean_loss, 'PoG_px_initial_unaugmented', 'PoG_px_tobii')
            term('metric_euc_PoG_cm_initial_unaugmented', losses.euclidean_loss, 'PoG_cm_initial_unaugmented', 'PoG_cm_tobii')
            term('metric_ang_g_initial_unaugmented', losses.angular_loss, 'g_initial_unaugmented', 'g')
        for stage in ('initial', 'final'):
            term('loss_mse_PoG_px_' + stage, losses.mse_loss, 'PoG_px_' + stage, 'PoG_px_tobii')
            term('metric_euc_PoG_px_' + stage, losses.euclidean_loss, 'PoG_px_' + stage, 'PoG_px_tobii')
            term('loss_mse_PoG_cm_' + stage, losses.mse_loss, 'PoG_cm_' + stage, 'PoG_cm_tobii')
            term('metric_euc_PoG_cm_' + stage, losses.euclidean_loss, 'PoG_cm_' + stage, 'PoG_cm_tobii')
            term('metric_ang_g_' + stage, losses.angular_loss, 'g_' + stage, 'g')
        if batched:
            vals = ops.VectorTermsFn.apply(tuple((kind, tgt, val) for _, kind, _, tgt, val in batched), *[b[2] for b in batched])
            for (name, _, _, _, _), v in zip(batched, vals):
                out[name] = v

    def _full_loss(self, out, device):                                # eve.py:234-265
        cfg = self.config
        total = torch.zeros((), device=device)
        if 'loss_ang_left_g_initial' in out:
            total = total + cfg.loss_coeff_g_ang_initial * (out['loss_ang_left_g_initial'] + out['loss_ang_right_g_initial'])
        if 'loss_mse_left_PoG_cm_initial' in out and cfg.loss_coeff_PoG_cm_initial > 0.0:
            total = total + cfg.loss_coeff_PoG_cm_initial * (out['loss_mse_left_PoG_cm_initial'] + out['loss_mse_right_PoG_cm_initial'])
        if 'loss_l1_left_pupil_size' in out:
            total = total + cfg.loss_coeff_pupil_size * (out['loss_l1_left_pupil_size'] + out['loss_l1_right_pupil_size'])
        if 'loss_mse_PoG_cm_final' in out:
            total = total + cfg.loss_coeff_PoG_cm_final * out['loss_mse_PoG_cm_final']
        if 'loss_ce_heatmap_initial' in out:
            total = total + cfg.loss_coeff_heatmap_ce_initial * out['loss_ce_heatmap_initial']
        if 'loss_ce_heatmap_final' in out:
            total = total + cfg.loss_coeff_heatmap_ce_final * out['loss_ce_heatmap_final']
        if 'loss_mse_heatmap_final' in out:
            total = total + cfg.loss_coeff_heatmap_mse_final * out['loss_mse_heatmap_final']
        return total
