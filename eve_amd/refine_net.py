"""RefineNet drop-in: 72x128 pre-activation U-Net with a conv-RNN bottleneck refining the point-of-gaze
heat-map, computed by the gfx950 HIP kernels of libeve_hip.so.

Mirrors /root/reference/src/models/refine_net.py:
  * `RefineNet()` (:179-235) reads the config singleton; sub-module names `initial`, `network`
    (`encoder_blocks`, `between_module`, `decoder_blocks`, `layers`, `skip_layer`, `rnn_cells.0.
    {gates_1,gate_2|gates|cell}`), `final` so state_dict keys equal the reference's;
    Kaiming fan_out init, IN weight 1 / bias 0, zero last conv weight (:226-235);
  * `forward(input_dict, output_dict, previous_output_dict=None) -> None` (:237-255): reads
    `output_dict['heatmap_initial']` (+ `input_dict['screen_frame']`), writes `heatmap_final` and
    `refinenet_rnn_states_0` (NCHW float at the boundary, like the reference);
  * Bottleneck quirks kept (:132-176): unknown rnn type => no cell; a tuple state (CLSTM) is stored but
    its output is NOT used downstream, so its weights get no gradient.  `refine_net_clstm_feeds_features = True`
    (an eve_amd config key, default False) departs from the reference on purpose: the cell's h becomes the features.

`forward_sequence` folds all T frames into the image batch for the encoder and decoder (InstanceNorm
is per-sample) and runs only the Cx5x8 conv-RNN cells sequentially (one clip-long scan per cell where `_use_scan` allows).
The cells themselves -- holders, one-frame step, clip scan, state dtype per kind -- live in conv_rnn.py; this module walks them.

nn.Conv2d / nn.InstanceNorm2d objects are PARAMETER HOLDERS; their ATen forward is never called.
"""

import torch
from torch import nn

from . import conv_rnn, ops
from .config import get_config
from .conv_rnn import CGRUCell, CLSTMCell, CRNNCell
from .eye_net import default_compute_dtype
from .kernels import ACT_LEAKY, ACT_NONE, ACT_RELU, default_kernels, pad_channels
from .ops import PackedWeight

# the screen key of a batch and its pixel format: a batch holds at most one (screen_frame is the float screen input or an
# RGB(A) capture, the others are what capture APIs, decoders and OpenCV deliver -- kernels.pixel_format_shape has the layouts);
# the mirror of eye_net.EYE_FRAME_KEYS
SCREEN_FRAME_KEYS = {'screen_frame': 'rgb', 'screen_frame_bgr': 'bgr', 'screen_frame_nv12': 'nv12', 'screen_frame_i420': 'i420',
                     'screen_frame_yuyv': 'yuyv'}


# one more screen key: the capture as a decoder's or capture API's surface lies in memory, uint8 [B, T, rows, pitch] or
# [B, T, frame_bytes], read through RefineNet.screen_layout (a data.SurfaceLayout); the mirror of eye_net.EYE_SURFACE_KEY
SCREEN_SURFACE_KEY = 'screen_surface'


def screen_frame_key(batch):
    """The one screen key of SCREEN_FRAME_KEYS (or SCREEN_SURFACE_KEY) the batch holds, or None; two of them raise ValueError."""
    found = [k_ for k_ in tuple(SCREEN_FRAME_KEYS) + (SCREEN_SURFACE_KEY,) if k_ in batch]
    if len(found) > 1:
        raise ValueError('give the screen under one key, not both: found %s' % ', '.join(found))
    return found[0] if found else None


def screen_capture(batch):
    """The keyword arguments RefineNet.forward_sequence / _stream_sequence take for the batch's screen beside screen_frame:
    {} or {its key: the capture} for one of the capture keys."""
    key = screen_frame_key(batch)
    return {} if key in (None, 'screen_frame') else {key: batch[key]}


class BasicBlock(nn.Module):     # holder, refine_net.py:35-62
    def __init__(self, in_shape, out_shape, act_func=nn.ReLU):
        super().__init__()
        ic, oc = in_shape[0], out_shape[0]
        assert tuple(in_shape[1:]) == tuple(out_shape[1:])
        self.act = ACT_LEAKY if act_func is nn.LeakyReLU else ACT_RELU
        self.layers = nn.Sequential(
            nn.InstanceNorm2d(ic, affine=True), act_func(inplace=True),
            nn.Conv2d(ic, oc, kernel_size=3, stride=1, padding=1),
            nn.InstanceNorm2d(oc, affine=True), act_func(inplace=True),
            nn.Conv2d(oc, oc, kernel_size=3, stride=1, padding=1))
        self.skip_layer = None
        if ic != oc:
            self.skip_layer = nn.Sequential(nn.InstanceNorm2d(ic, affine=True), act_func(inplace=True),
                                            nn.Conv2d(ic, oc, kernel_size=1, stride=1))


class WrapEncoderDecoder(nn.Module):   # holder, refine_net.py:70-113
    def __init__(self, in_shape, out_shape, module_to_wrap, add_skip_connection=False,
                 num_encoder_blocks=1, num_decoder_blocks=1):
        super().__init__()
        ic, ih, iw = in_shape
        oc, oh, ow = out_shape
        assert ih == oh and iw == ow
        self.in_shape, self.out_shape = in_shape, out_shape
        b_ic, bh, bw = module_to_wrap.in_shape
        b_oc = module_to_wrap.out_shape[0]
        self.inner_hw = (bh, bw)
        self.add_skip_connection = add_skip_connection
        self.encoder_blocks = nn.ModuleList(
            [BasicBlock([ic, ih, iw], [b_ic, ih, iw])] +
            [BasicBlock([b_ic, ih, iw], [b_ic, ih, iw]) for _ in range(num_encoder_blocks - 1)])
        self.downsample = nn.AdaptiveMaxPool2d([bh, bw]) if (ih, iw) != (bh, bw) else None
        self.between_module = module_to_wrap
        self.upsample = (nn.Upsample(size=[oh, ow], mode='bilinear', align_corners=False)
                         if (bh, bw) != (oh, ow) else None)
        dec_in = b_oc + (b_ic if add_skip_connection else 0)
        self.decoder_blocks = nn.ModuleList(
            [BasicBlock([dec_in, oh, ow], [oc, oh, ow], nn.LeakyReLU)] +
            [BasicBlock([oc, oh, ow], [oc, oh, ow], nn.LeakyReLU) for _ in range(num_decoder_blocks - 1)])


class Bottleneck(nn.Module):     # holder, refine_net.py:132-152
    def __init__(self, tensor_shape, config):
        super().__init__()
        self.in_shape = self.out_shape = tensor_shape
        if config.refine_net_use_rnn:
            kinds = {'CRNN': CRNNCell, 'CLSTM': CLSTMCell, 'CGRU': CGRUCell}
            cells = []
            for _ in range(config.refine_net_rnn_num_cells):
                if config.refine_net_rnn_type in kinds:
                    cells.append(kinds[config.refine_net_rnn_type](
                        input_size=config.refine_net_num_features,
                        hidden_size=config.refine_net_num_features))
            self.rnn_cells = nn.ModuleList(cells)


class RefineNet(nn.Module):
    LEVELS = [(256, 5, 8, 2), (128, 9, 16, 2), (64, 18, 32, 2), (32, 36, 64, 2), (16, 72, 128, 1)]

    def __init__(self):
        super(RefineNet, self).__init__()
        config = get_config()
        self.config = config
        self.compute_dtype = default_compute_dtype()
        self.in_c = 4 if config.load_screen_content else 1
        skip = config.refine_net_use_skip_connections
        wrapped = Bottleneck((config.refine_net_num_features, 5, 8), config)
        for c, h, w, n_enc in self.LEVELS:
            wrapped = WrapEncoderDecoder([c, h, w], [c, h, w], wrapped, add_skip_connection=skip,
                                         num_encoder_blocks=n_enc)
        self.initial = nn.Sequential(
            nn.Conv2d(self.in_c, 16, kernel_size=3, padding=1), nn.InstanceNorm2d(16, affine=True),
            nn.ReLU(inplace=True), nn.Conv2d(16, 16, kernel_size=3, padding=1))
        self.network = wrapped
        self.final = nn.Sequential(
            nn.Conv2d(16, 16, kernel_size=3, padding=1), nn.LeakyReLU(inplace=True),
            nn.Conv2d(16, 1, kernel_size=1), nn.Sigmoid())
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.InstanceNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        nn.init.zeros_(self.final[-2].weight)
        self._packs = None
        self._packs_key = None
        self._probe = None          # test hook: callable(name, NHWC tensor) -> tensor at every stage boundary

    def _tap(self, name, x):
        return x if self._probe is None else self._probe(name, x)

    # ------------------------------------------------------------------ packed weights
    def invalidate_packs(self):
        self._packs = None

    def _get_packs(self):
        dt = self.compute_dtype
        key = (dt,) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packs is not None and self._packs_key == key:
            return self._packs
        P = {}
        for name, m in self.named_modules():
            if isinstance(m, nn.Conv2d):
                cin_pad = pad_channels(m.in_channels, dt)
                cout_pad = pad_channels(m.out_channels, dt)
                P[name] = PackedWeight(m.weight, dt, cin_pad=cin_pad, cout_pad=cout_pad, defer=True)
        PackedWeight.pack_many(list(P.values()), dt)      # every filter bank of the network in one launch per 48 (was one each)
        self._packs, self._packs_key = P, key
        return P

    def _conv(self, x, name, m, P, act=ACT_NONE, acc=None, want_stats=False):
        return ops.conv2d(x, m.weight, m.bias, P[name], stride=1, pad=m.padding[0], act=act, acc=acc, want_stats=want_stats)

    # ------------------------------------------------------------------ blocks
    def _block(self, x, blk, prefix, P):
        """x: the block input, or a tuple of NHWC sources whose channel-concatenation is the block input (the decoder's
        torch.cat of refine_net.py:125-126, which is then never materialised)."""
        L, S = blk.layers, blk.skip_layer
        xs = x if isinstance(x, tuple) else (x,)
        # both heads of a block with a skip convolution normalise the same input: one statistics pass and one read per source,
        # each head written into its channel range (planes too large for the register-resident kernel; small ones keep it)
        two_heads = S is not None and all(t.shape[1] * t.shape[2] * t.shape[3] > 65536 for t in xs)
        if two_heads:
            a, skip = ops.instnorm_act2(xs, L[0].weight, L[0].bias, S[0].weight, S[0].bias, act=blk.act)
        else:
            x = xs[0] if len(xs) == 1 else torch.cat(xs, dim=-1)
            if S is None and torch.is_grad_enabled() and x.requires_grad and hasattr(ops, 'InstNormActSkipFn'):
                # identity skip: x feeds `layers` and the final add -- one node, the two gradients meet in its backward
                a, skip = ops.InstNormActSkipFn.apply(x, L[0].weight, L[0].bias, blk.act, 1e-5)
            else:
                a = ops.instnorm_act(x, L[0].weight, L[0].bias, act=blk.act)
                skip = x if S is None else ops.instnorm_act(x, S[0].weight, S[0].bias, act=blk.act)
        # the mid-block InstanceNorm's statistics come out of the convolution's own epilogue where its kernel walks whole
        # images (the row-streaming 3x3 kernel of the two outer levels): no statistics pass over the plane
        a, mr = self._conv(a, prefix + '.layers.2', L[2], P, want_stats=True)
        a = ops.instnorm_act(a, L[3].weight, L[3].bias, act=blk.act, stats=mr)
        a = self._conv(a, prefix + '.layers.5', L[5], P)
        if S is not None:           # layers(x) + skip_layer(x): the 1x1 convolution accumulates into the 3x3 branch's output
            return self._conv(skip, prefix + '.skip_layer.2', S[2], P, acc=a)
        return ops.add(a, skip)

    def _encode(self, x, P):
        """Runs `initial` and every level's encoder on the folded frame batch.
        Returns the bottleneck input and the per-level encoder outputs (outermost first)."""
        x = self._tap('input', x)
        x = self._conv(x, 'initial.0', self.initial[0], P)
        x = ops.instnorm_act(x, self.initial[1].weight, self.initial[1].bias, act=ACT_RELU)
        x = self._tap('initial', self._conv(x, 'initial.3', self.initial[3], P))
        skips, level, prefix, depth = [], self.network, 'network', 0
        while isinstance(level, WrapEncoderDecoder):
            for i, blk in enumerate(level.encoder_blocks):
                x = self._tap('enc%d.%d' % (depth, i), self._block(x, blk, '%s.encoder_blocks.%d' % (prefix, i), P))
            if level.downsample is not None and level.add_skip_connection and torch.is_grad_enabled() and x.requires_grad:
                # the level's output goes to the pool and to the decoder's skip: one node, their gradients meet in its backward
                pooled, x_skip = ops.PoolForkFn.apply(x, tuple(level.inner_hw))
                skips.append(x_skip)
                x = self._tap('pool%d' % depth, pooled)
            else:
                skips.append(x)
                if level.downsample is not None:
                    x = self._tap('pool%d' % depth, ops.AdaptiveMaxPoolFn.apply(x, tuple(level.inner_hw)))
            level, prefix, depth = level.between_module, prefix + '.between_module', depth + 1
        return x, skips, prefix

    def _decode(self, x, skips, P):
        levels, level, prefix = [], self.network, 'network'
        while isinstance(level, WrapEncoderDecoder):
            levels.append((level, prefix))
            level, prefix = level.between_module, prefix + '.between_module'
        for depth, (level, prefix), enc in zip(reversed(range(len(levels))), reversed(levels), reversed(skips)):
            if level.upsample is not None:
                x = self._tap('up%d' % depth, ops.BilinearFn.apply(x, (level.out_shape[1], level.out_shape[2])))
            if level.add_skip_connection:
                x = (x, enc)                                   # concatenated by the first decoder block's InstanceNorms
            for i, blk in enumerate(level.decoder_blocks):
                x = self._tap('dec%d.%d' % (depth, i), self._block(x, blk, '%s.decoder_blocks.%d' % (prefix, i), P))
        x = self._tap('final0', self._conv(x, 'final.0', self.final[0], P, act=ACT_LEAKY))
        # logits of the last 1x1 convolution (channel 0); the sigmoid is evaluated in float by the head kernel
        logits = self._tap('logits', self._conv(x, 'final.2', self.final[2], P))
        return ops.HeatmapHeadFn.apply(logits)                                 # [N, 1, H, W] float

    # ------------------------------------------------------------------ conv-RNN bottleneck, one step
    def _clstm_live(self):
        """config.refine_net_clstm_feeds_features (eve_amd only; absent from the reference's config singleton => False): a
        tuple state's h becomes the bottleneck features instead of being stored and dropped (refine_net.py:168-174)."""
        return bool(getattr(self.config, 'refine_net_clstm_feeds_features', False))

    def _cell_step(self, x, state, cell, prefix, P):
        """x: [B,5,8,C] NHWC.  state: previous state (tensor, or (h, c) for CLSTM) or None.
        Returns (features for the decoder, new state)."""
        return cell.step(self._conv, x, state, prefix, P, self._clstm_live())

    def _rnn_cells(self):
        bott = self.network
        while isinstance(bott, WrapEncoderDecoder):
            bott = bott.between_module
        return list(bott.rnn_cells) if self.config.refine_net_use_rnn else []

    def _bottleneck(self, x, states, prefix, P):
        """x: [B,5,8,C].  states: list (one per cell) of previous states or None.  -> (x, new states)"""
        new_states = []
        for i, cell in enumerate(self._rnn_cells()):
            prev = None if states is None else states[i]
            x, st = self._cell_step(x, prev, cell, '%s.rnn_cells.%d' % (prefix, i), P)
            new_states.append(st)
        return x, new_states

    # ------------------------------------------------------------------ boundary helpers
    def _input_nhwc(self, heatmap, screen):
        cfg, dt = self.config, self.compute_dtype
        H, W = cfg.screen_size[1], cfg.screen_size[0]
        if tuple(heatmap.shape[-2:]) != (H, W):       # F.interpolate(..., bilinear) of refine_net.py:240-243
            hm = ops.ToNHWCFn.apply(heatmap, dt, pad_channels(1, dt))
            hm = ops.BilinearFn.apply(hm, (H, W))
            heatmap = ops.FromNHWCFn.apply(hm, 1)
        x = torch.cat([screen, heatmap], dim=1) if cfg.load_screen_content else heatmap
        return ops.ToNHWCFn.apply(x, dt, pad_channels(x.shape[1], dt))

    def _state_in(self, st):
        dt = self.compute_dtype
        f = lambda t: ops.ToNHWCFn.apply(t, dt, pad_channels(t.shape[1], dt))
        return tuple(f(t) for t in st) if isinstance(st, tuple) else f(st)

    @staticmethod
    def _state_out(st):
        f = lambda t: ops.FromNHWCFn.apply(t, t.shape[-1])
        return tuple(f(t) for t in st) if isinstance(st, tuple) else f(st)

    # ------------------------------------------------------------------ reference per-step contract
    def forward(self, input_dict, output_dict, previous_output_dict=None):
        P = self._get_packs()
        screen = input_dict['screen_frame'] if self.config.load_screen_content else None
        x = self._input_nhwc(output_dict['heatmap_initial'], screen)
        x, skips, prefix = self._encode(x, P)
        states = None
        if previous_output_dict is not None:
            states = [self._state_in(previous_output_dict['refinenet_rnn_states_%d' % i])
                      for i in range(len(self._rnn_cells()))]
        x, new_states = self._bottleneck(x, states, prefix, P)
        for i, st in enumerate(new_states):
            output_dict['refinenet_rnn_states_%d' % i] = self._state_out(st)
        y = self._decode(x, skips, P)
        output_dict['heatmap_final'] = y

    # ------------------------------------------------------------------ whole clips in one pass
    _use_scan = staticmethod(conv_rnn.use_scan)         # (cells, (h, w, C), dtype) -> clip scans or the per-frame loop

    def _carried_dtypes(self):
        """Per cell, the dtype(s) the bottleneck carries its state in (internal NHWC layout [B, 5, 8, C]); a pair for CLSTM."""
        cells, dt = self._rnn_cells(), self.compute_dtype
        scan = self._use_scan(cells, (5, 8, pad_channels(self.config.refine_net_num_features, dt)), dt)
        return [cell.state_dtypes(scan, dt) for cell in cells]

    def _initial_states_in(self, initial_states):
        """initial_states: None, or one entry per cell -- a state (a pair for CLSTM) in the reference layout [B, C, 5, 8] (what
        `forward` / `forward_sequence` return) or in the internal NHWC layout [B, 5, 8, C] (EVEStream's carried buffers), or
        None for a zero state.  -> per cell the internal-layout tensor(s) in the dtype the bottleneck carries."""
        if initial_states is None:
            return None
        dts = self._carried_dtypes()
        assert len(initial_states) == len(dts), 'initial_states: one entry per RefineNet cell (%d)' % len(dts)
        C = self.config.refine_net_num_features

        def one(t, sdt):
            if t.dim() == 4 and t.shape[1] == C and tuple(t.shape[2:]) == (5, 8) and t.shape[-1] != C:
                t = self._state_in(t)                       # reference NCHW -> NHWC, compute dtype
            return t if t.dtype == sdt and t.is_contiguous() else t.to(sdt).contiguous()

        out = []
        for st, sdt in zip(initial_states, dts):
            if st is None:
                out.append(None)
            elif isinstance(sdt, tuple):
                out.append(tuple(one(t, d) for t, d in zip(st, sdt)))
            else:
                out.append(one(st, sdt))
        return out

    # The YUV -> RGB matrix of screen_frame_nv12 / _i420 / _yuyv captures: 'bt601' (limited range: OpenCV's cvtColor, SD video),
    # 'bt709' (limited range: what HD recordings and hardware decoders of HD video usually are) or 'jfif' (full range).  Anything
    # else raises ValueError at use.
    yuv_matrix = 'bt601'
    # How screen_surface captures lie in memory: a data.SurfaceLayout (format, visible size, pitch, coded rows, crop origin, plane
    # offsets).  A screen_surface capture without it raises ValueError.
    screen_layout = None

    def forward_sequence(self, heatmap_initial, screen_frame=None, initial_states=None, screen_frame_bgr=None, screen_frame_nv12=None,
                         screen_frame_i420=None, screen_frame_yuyv=None, screen_surface=None):
        """heatmap_initial [B,T,1,h,w], screen_frame [B,T,3,H,W] -> (heatmap_final [B,T,1,H,W],
        list over cells of the stacked states [B,T,C,5,8] (tuple of two for CLSTM)).
        screen_frame may also be uint8 [B,T,IH,IW,3|4]: decoded frames at the screen size, or a full-resolution capture that is
        area-averaged down to config.screen_size on the device (data.preprocess_screen_frames; channel order kept, alpha ignored).
        screen_frame_bgr: in place of screen_frame, a uint8 [B,T,IH,IW,3|4] BGR(A) capture as capture APIs and OpenCV deliver it;
        the result is that of the channel-reversed capture as screen_frame, bit for bit.  Both together raise ValueError.
        screen_frame_nv12 / screen_frame_i420 (uint8 [B,T,IH*3/2,IW], IH and IW even) / screen_frame_yuyv (uint8 [B,T,IH,IW,2], IW
        even): in place of screen_frame, the capture as a decoder or a capture path delivers it; every pixel is converted by the
        integer matrix self.yuv_matrix names as the area resize reads it (eve_screen_area_fmt_to_nchw), and the result is that of
        the converted RGB capture as screen_frame, bit for bit.  One screen argument at a time: two raise ValueError.
        screen_surface (uint8 [B,T,rows,pitch] or [B,T,frame_bytes]): in place of screen_frame, the capture as a decoder's or capture
        API's surface lies in memory -- pitched rows, coded rows, a window of a larger texture, NV21 / YV12 / UYVY / P010 / pitched
        BGRA -- read through self.screen_layout, a data.SurfaceLayout (eve_screen_area_surface_to_nchw): the result is that of the
        de-pitched, cropped, byte-linear capture under its format's key, bit for bit.
        initial_states: None (zero states), or per cell the state before the first frame -- reference layout [B, C, 5, 8] as
        returned here (the last frame of a previous call), or the internal NHWC layout [B, 5, 8, C]; (h, c) for CLSTM."""
        screen_frame = self._screen_input(screen_frame, screen_frame_bgr=screen_frame_bgr, screen_frame_nv12=screen_frame_nv12,
                                          screen_frame_i420=screen_frame_i420, screen_frame_yuyv=screen_frame_yuyv,
                                          screen_surface=screen_surface)
        hf, states, to_ref = self._sequence(heatmap_initial, screen_frame, self._initial_states_in(initial_states))
        return hf, [tuple(to_ref(t) for t in st) if isinstance(st, tuple) else to_ref(st) for st in states]

    def _screen_input(self, screen_frame, **captures):
        """screen_frame as it is, or the float [B,T,3,H,W] screen input made from the one capture given under a key of
        SCREEN_FRAME_KEYS other than screen_frame -- BGR(A), NV12, I420 or YUYV (one area-resize launch)."""
        given = {k_: v for k_, v in captures.items() if v is not None}
        assert all((k_ in SCREEN_FRAME_KEYS and k_ != 'screen_frame') or k_ == SCREEN_SURFACE_KEY for k_ in given), sorted(given)
        if not given:
            return screen_frame
        if screen_frame is not None or len(given) > 1:
            raise ValueError('give the screen as screen_frame or under one of %s, not both' % ', '.join(
                [k_ for k_ in SCREEN_FRAME_KEYS if k_ != 'screen_frame'] + [SCREEN_SURFACE_KEY]))
        (key, capture), = given.items()
        from . import data
        cfg = self.config
        size = (cfg.screen_size[1], cfg.screen_size[0])
        if key == 'screen_frame_bgr':
            if not torch.is_tensor(capture) or capture.dtype != torch.uint8 or capture.dim() != 5 or capture.shape[4] not in (3, 4):
                raise TypeError('screen_frame_bgr must be uint8 [B, T, IH, IW, 3 | 4], got %s %s' % (
                    getattr(capture, 'dtype', type(capture)), tuple(getattr(capture, 'shape', ()))))
            return data.preprocess_screen_frames(capture, size=size, bgr=True)
        from .kernels import YUV_MATRICES, pixel_format_shape
        if key == SCREEN_SURFACE_KEY:
            if self.screen_layout is None:
                raise ValueError('%s needs RefineNet.screen_layout, a data.SurfaceLayout that says how the capture lies in memory' % key)
            if self.yuv_matrix not in YUV_MATRICES:
                raise ValueError('RefineNet.yuv_matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), self.yuv_matrix))
            flat, lead = data.surface_frames(capture, self.screen_layout, 2, name=key)
            out = data.preprocess_screen_frames(flat, size=size, layout=self.screen_layout, matrix=self.yuv_matrix)
            return out.view(lead + tuple(out.shape[1:]))
        pixel_format_shape(capture, SCREEN_FRAME_KEYS[key], lead=2, name=key)
        if self.yuv_matrix not in YUV_MATRICES:
            raise ValueError('RefineNet.yuv_matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), self.yuv_matrix))
        return data.preprocess_screen_frames(capture, size=size, format=SCREEN_FRAME_KEYS[key], matrix=self.yuv_matrix)

    def _sequence(self, heatmap_initial, screen_frame, h0, plan=None):
        """The clip pass behind forward_sequence.  h0: None or per cell the internal-layout initial state (_initial_states_in).
        plan: None, or kernels.stream_mask_plan's result (a masked EVEStream step): the bottleneck input is gathered through the
        frame sequences' perm, so the cells see every stream's valid frames first and in order, and the last cell's features are
        gathered back through inv before the decoder; the per-frame states returned are then in the compacted order.
        Returns (heatmap_final [B,T,1,H,W], per cell its per-frame states [B,T,5,8,C] (a pair for CLSTM), to_ref); to_ref
        converts [B,T,5,8,C] to [B,T,C,5,8]."""
        P = self._get_packs()
        B, T = heatmap_initial.shape[:2]
        if screen_frame is not None and screen_frame.dtype == torch.uint8:     # decoded frames [B,T,H,W,3]: normalise here
            from . import data                                                 # (a full-resolution capture [B,T,IH,IW,3|4]: area-resized too)
            cfg = self.config
            screen_frame = data.preprocess_screen_frames(screen_frame, size=(cfg.screen_size[1], cfg.screen_size[0]))
        fold = lambda t: None if t is None else t.reshape((B * T,) + tuple(t.shape[2:]))
        x = self._input_nhwc(fold(heatmap_initial), fold(screen_frame) if self.config.load_screen_content else None)
        x, skips, prefix = self._encode(x, P)
        h5, w5, C = x.shape[1:]
        xs = x.view(B, T, h5, w5, C)
        if plan is not None:
            xs = default_kernels().stream_permute_rows(xs, plan['perm'][2 * B:])
        cells, live = self._rnn_cells(), self._clstm_live()
        to_ref = lambda t: ops.FromNHWCFn.apply(t.reshape(B * T, h5, w5, C), C).view(B, T, C, h5, w5)
        if self._use_scan(cells, xs.shape[2:], xs.dtype):
            # a stack is cell 0 scanned over the clip, then cell 1 over cell 0's states, ...: cell i at frame t reads cell i-1 at
            # frame t and its own state at t-1, which is all the per-frame loop of refine_net.py:154-176 does
            states, hs = [], xs
            for i, cell in enumerate(cells):
                st, hs = cell.scan(hs, None if h0 is None else h0[i], '%s.rnn_cells.%d' % (prefix, i), P, live)
                states.append(st)
        else:
            outs, prev, hist = [], h0, []
            for t in range(T):
                xt, prev = self._bottleneck(xs[:, t].contiguous(), prev, prefix, P)
                outs.append(xt)
                hist.append(prev)
            hs = torch.stack(outs, dim=1)
            stack = lambda ts: torch.stack(ts, dim=1)           # a cell's per-frame states as a scan returns them: [B,T,5,8,C]
            states = [tuple(map(stack, zip(*per_t))) if isinstance(per_t[0], tuple) else stack(per_t) for per_t in zip(*hist)]
        if plan is not None:
            hs = default_kernels().stream_permute_rows(hs, plan['inv'][2 * B:])
        x = hs.reshape(B * T, h5, w5, C)
        if cells:
            x = self._tap('rnn', x)
        hf = self._decode(x, skips, P)
        return hf.view(B, T, 1, hf.shape[2], hf.shape[3]), states, to_ref

    # ------------------------------------------------------------------ streaming (eve_amd/stream.py)
    def _stream_state_buffers(self, B, device):
        """Zero-initialised carried states for B streams, one per cell (a pair for CLSTM), in the internal layout and dtype."""
        C = pad_channels(self.config.refine_net_num_features, self.compute_dtype)
        z = lambda dt: torch.zeros((B, 5, 8, C), dtype=dt, device=device)
        return [tuple(z(d) for d in dt) if isinstance(dt, tuple) else z(dt) for dt in self._carried_dtypes()]

    def _stream_sequence(self, heatmap_initial, screen_frame, buffers, reset=None, lengths=None, plan=None, **captures):
        """One chunk of a stream: the carried states `buffers` (from _stream_state_buffers) are zeroed where reset[b] != 0, used
        as the initial states, and overwritten with the chunk's last frame -- one eve_stream_state_rows launch each way, no
        conversion.  lengths (None, or int32 [B] on the device): stream b's states are committed from its frame lengths[b] - 1
        instead (eve_stream_state_rows_at), or kept when that is 0.  plan (None, or kernels.stream_mask_plan's result, which holds
        the lengths already): stream b consumes exactly its valid frames -- _sequence compacts them to the front, and the states
        are committed from the last valid one (the plan's frame counts as lengths), held when there is none; heatmap_final at
        the other frames is unspecified.  captures: the screen under one of forward_sequence's capture keywords (screen_frame_bgr,
        _nv12, _i420, _yuyv) in place of screen_frame.  -> heatmap_final [B,T,1,H,W]."""
        k = default_kernels()
        flat = lambda sts: [t for s in sts for t in (s if isinstance(s, tuple) else (s,))]
        if reset is not None:
            for t in flat(buffers):
                k.stream_state_rows(t, t, reset)
        if plan is not None:
            lengths = plan['count'][2 * heatmap_initial.shape[0]:]
        screen_frame = self._screen_input(screen_frame, **captures)
        hf, states, _ = self._sequence(heatmap_initial, screen_frame, buffers if buffers else None, plan)
        for dst, src in zip(flat(buffers), flat(states)):
            if lengths is None:
                k.stream_state_rows(src[:, -1], dst)
            else:
                k.stream_state_rows_at(src, dst, lengths)
        return hf
