"""RefineNet's conv-RNN cells (CRNN / CLSTM / CGRU on the C x 5 x 8 bottleneck, common.py:331-415): per kind the parameter
holder, its one-frame step, its clip-long scan, the dtype it carries its state in, and the autograd shells under them.
refine_net.py owns the U-Net around the cells and walks them; nothing outside this module knows one kind from another.
Activations and states are NHWC: one frame [B, 5, 8, C], a clip [B, T, 5, 8, C], time-major ("_tm") [T, B, 5, 8, C]."""

import torch
from torch import nn

from .kernels import ACT_TANH, HALF_DTYPES, SCAN_WIDTHS, default_kernels, dispatch_flag
from .ops import _bias_grad_into, _wgrad_into


def _float_banks(weight, pack):
    """(OHWI, IHWO) float32 copies of a convolution's filter bank for the float32 clip scans (csrc/cell_scan_f32.hip): the
    pack's own tensors in the float32 instantiation, otherwise formed from the parameter (295-590 KB)."""
    if pack is not None and pack.ohwi.dtype == torch.float32 and pack.ihwo is not None:
        return pack.ohwi, pack.ihwo
    w = weight.detach().float()
    return w.permute(0, 2, 3, 1).contiguous(), w.permute(1, 2, 3, 0).contiguous()


def _f32(t):        # what the float32 scans take for a bias or an initial state (None stays None)
    return None if t is None else t.detach().float().contiguous()


def _bank_grads(k, xs_tm, h0, hs_tm, dpre, w, b, pack, need_w, need_b, operand_tm=None):
    """Weight and bias gradient of a scanned cell's 3x3 gate convolution: ONE batched launch each over all T*B frames.
    dpre [T, B, H, W, G] is the gradient of its output; what it read per frame is [x_t | h_{t-1}] -- hs_tm shifted one frame
    behind the initial state h0 (None: zeros) -- unless operand_tm [T, B, H, W, 2C] says otherwise (CGRU's [r*h | x])."""
    if operand_tm is None:
        first = h0 if h0 is not None else torch.zeros_like(hs_tm[0])
        operand_tm = torch.cat([xs_tm, torch.cat([first.unsqueeze(0), hs_tm[:-1]], dim=0)], dim=-1)
    T, B, H, W = dpre.shape[:4]
    operand, gpre = operand_tm.reshape(T * B, H, W, -1), dpre.view(T * B, H, W, -1)
    dw = _wgrad_into(k, operand, gpre, w, pack, 1, 1) if need_w else None
    db = _bias_grad_into(k, gpre, b) if need_b else None
    return dw, db


class CGRUGates1Fn(torch.autograd.Function):
    """(ru, rh) = (sigmoid(g1), sigmoid(g1[..., :C]) * h)   -- common.py:410-411"""

    @staticmethod
    def forward(ctx, g1, h):
        ru, rh = default_kernels().cgru_gates1(g1, h)
        ctx.save_for_backward(ru, h)
        return ru, rh

    @staticmethod
    def backward(ctx, dru, drh):
        ru, h = ctx.saved_tensors
        dg1, dh = default_kernels().cgru_gates1_bwd(drh.contiguous(), dru.contiguous(), ru, h)
        return dg1, dh


class CGRUGates2Fn(torch.autograd.Function):
    """h' = (1 - u) * tanh(g2) + u * h   -- common.py:413-414.  `ru` only contributes through u."""

    @staticmethod
    def forward(ctx, g2, ru, h):
        o, hnew = default_kernels().cgru_gates2(g2, ru, h)
        ctx.save_for_backward(ru, h, o)
        return hnew

    @staticmethod
    def backward(ctx, dhnew):
        ru, h, o = ctx.saved_tensors
        dg2, dru, dh = default_kernels().cgru_gates2_bwd(dhnew.contiguous(), ru, h, o)
        return dg2, dru, dh


class CGRUScanFn(torch.autograd.Function):
    """hs[:, t] = CGRUCell(xs[:, t], hs[:, t-1]) for the whole clip in ONE launch (kernels.cgru_scan_fwd: hidden state
    resident in LDS, both gate convolutions and their sigmoid / tanh / blend epilogues fused; common.py:388-415 applied
    per frame by refine_net.py:132-176).  The backward is one persistent launch as well (kernels.cgru_scan_bwd: frames in
    reverse, gate gradients + both data-gradient GEMMs + the carry into the previous state fused; eve_dispatch_config.cgru_scan = 2
    selects the per-frame kernels on time-major tensors); the two weight gradients and bias gradients are ONE batched
    launch each over all T*B frames."""

    @staticmethod
    def forward(ctx, xs, w1, b1, w2, b2, h0, p1, p2):
        k = default_kernels()
        h0c = h0.detach().contiguous() if h0 is not None else None
        hs, hs_tm, ru, rh, og = k.cgru_scan_fwd(xs.contiguous(), h0c, p1.ohwi, _f32(b1), p2.ohwi, _f32(b2))
        ctx.packs = (p1, p2)
        ctx.params = (w1, b1, w2, b2)
        ctx.has_h0 = h0 is not None
        ctx.save_for_backward(xs, h0c, hs_tm, ru, rh, og)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        k = default_kernels()
        xs, h0, hs_tm, ru, rh, og = ctx.saved_tensors
        p1, p2 = ctx.packs
        w1, b1, w2, b2 = ctx.params
        B, T, H, W, C = xs.shape
        need = ctx.needs_input_grad
        dhs_tm = dhs.transpose(0, 1).contiguous()                       # [T, B, ...]
        xs_tm = xs.transpose(0, 1).contiguous()
        want_dh0 = bool(ctx.has_h0 and need[5])
        if hasattr(k, 'cgru_scan_bwd') and dispatch_flag(k, 'cgru_scan', 1) != 2:
            # the whole frame-reversed recursion in one persistent launch (kernels.cgru_scan_bwd): gate gradients, both
            # data-gradient GEMMs, the carry into the previous state; gradients of the two pre-activations come back for
            # the batched weight / bias gradients below
            dg1_all, dg2_all, dxs_tm, dh0 = k.cgru_scan_bwd(dhs_tm, ru, og, hs_tm, h0, p1.ihwo, p2.ihwo, want_dh0)
            dxs = dxs_tm.transpose(0, 1).contiguous()
        else:
            first = h0 if h0 is not None else torch.zeros_like(xs_tm[0])
            dcat1_all = torch.empty((T, B, H, W, 2 * C), dtype=xs.dtype, device=xs.device)      # d[x | h] per frame
            dcat2_all = torch.empty((T, B, H, W, 2 * C), dtype=xs.dtype, device=xs.device)      # d[r*h | x] per frame
            dg1_all = torch.empty((T, B, H, W, 2 * C), dtype=xs.dtype, device=xs.device)
            dg2_all = torch.empty((T, B, H, W, C), dtype=xs.dtype, device=xs.device)
            carry = None
            for t in range(T - 1, -1, -1):
                dhn = dhs_tm[t] if carry is None else k.add(dhs_tm[t], carry)
                h_prev = hs_tm[t - 1] if t > 0 else first
                dg2, dru, dh_a = k.cgru_gates2_bwd(dhn, ru[t], h_prev, og[t])
                dcat2 = k.conv2d_dgrad(dg2, p2.ihwo, (H, W), 1, 1, algo=p2.algo)
                dg1, dh_b = k.cgru_gates1_bwd(dcat2[..., :C].contiguous(), dru, ru[t], h_prev)
                dcat1 = k.conv2d_dgrad(dg1, p1.ihwo, (H, W), 1, 1, algo=p1.algo)
                carry = k.add(k.add(dh_a, dh_b), dcat1[..., C:].contiguous())
                dcat1_all[t], dcat2_all[t], dg1_all[t], dg2_all[t] = dcat1, dcat2, dg1, dg2
            # d(xs) = x-halves of the two concatenated-input gradients, for all frames at once
            dxs = (dcat1_all[..., :C] + dcat2_all[..., C:]).transpose(0, 1).contiguous()
            dh0 = carry if want_dh0 else None
        dw1, db1 = _bank_grads(k, xs_tm, h0, hs_tm, dg1_all, w1, b1, p1, need[1], need[2])
        dw2, db2 = _bank_grads(k, xs_tm, h0, hs_tm, dg2_all, w2, b2, p2, need[3], need[4], torch.cat([rh, xs_tm], dim=-1))
        return dxs, dw1, db1, dw2, db2, dh0, None, None


class CRNNScanFn(torch.autograd.Function):
    """hs[:, t] = CRNNCell(xs[:, t], hs[:, t-1]) = tanh(conv3x3([x_t | h_{t-1}]) + b) for the whole clip in ONE launch, and the
    frame-reversed backward in one more (kernels.crnn_scan_{fwd,bwd}, float32: csrc/cell_scan_f32.hip; common.py:331-352 applied
    per frame by refine_net.py:132-176).  The weight and bias gradients are one batched launch each over all T*B frames.
    xs float32 [B, T, 5, 8, C], C in kernels.SCAN_WIDTHS (16-bit callers convert: the bottleneck is 40 C values per frame)."""

    @staticmethod
    def forward(ctx, xs, w, b, h0, pack):
        k = default_kernels()
        h0c = h0.detach().contiguous() if h0 is not None else None
        w_ohwi, w_ihwo = _float_banks(w, pack)
        xs = xs.contiguous()
        hs, hs_tm = k.crnn_scan_fwd(xs, h0c, w_ohwi, _f32(b))
        ctx.pack = pack
        ctx.params = (w, b)
        ctx.has_h0 = h0 is not None
        ctx.save_for_backward(xs, h0c, hs_tm, w_ihwo)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        k = default_kernels()
        xs, h0, hs_tm, w_ihwo = ctx.saved_tensors
        w, b = ctx.params
        need = ctx.needs_input_grad
        dhs_tm = dhs.float().transpose(0, 1).contiguous()
        want_dh0 = bool(ctx.has_h0 and need[3])
        dpre, dxs_tm, dh0 = k.crnn_scan_bwd(dhs_tm, hs_tm, w_ihwo, want_dh0)
        dxs = dxs_tm.transpose(0, 1).contiguous() if need[0] else None
        dw, db = _bank_grads(k, xs.transpose(0, 1), h0, hs_tm, dpre, w, b, ctx.pack, need[1], need[2])
        return dxs, dw, db, dh0, None


def clstm_scan(xs, weight, bias, pack, h0=None, c0=None):
    """CLSTMCell over a clip in one launch, forward only (kernels.clstm_scan_fwd; common.py:355-385): the reference stores
    the (h, c) tuple and never feeds it to the decoder (refine_net.py:168-174), so nothing is differentiated.  Also what the live
    cell (CLSTMScanFn) runs under torch.no_grad(): the training forward gives the same hs / cs bit for bit.
    xs [B, T, 5, 8, C] any dtype -> (hs, cs) float32 [B, T, 5, 8, C]."""
    k = default_kernels()
    with torch.no_grad():
        w_ohwi, _ = _float_banks(weight, pack)
        return k.clstm_scan_fwd(_f32(xs), _f32(h0), _f32(c0), w_ohwi, _f32(bias))


class CLSTMScanFn(torch.autograd.Function):
    """(hs, cs)[:, t] = CLSTMCell(xs[:, t], (hs, cs)[:, t-1]) for the whole clip in ONE launch, differentiable: what
    refine_net_clstm_feeds_features = True runs (the reference never feeds a tuple state on, so it has nothing to differentiate
    -- that path stays on clstm_scan).  kernels.clstm_scan_fwd_train gives the hs / cs of clstm_scan_fwd bit for bit and keeps
    the gates; kernels.clstm_scan_bwd walks the frames in reverse in one more launch; like CRNNScanFn the weight and bias
    gradients are one batched launch each over all T*B frames.  xs float32 [B, T, 5, 8, C], C in kernels.SCAN_WIDTHS."""

    @staticmethod
    def forward(ctx, xs, w, b, h0, c0, pack):
        k = default_kernels()
        h0c, c0c = _f32(h0), _f32(c0)
        w_ohwi, w_ihwo = _float_banks(w, pack)
        xs = xs.contiguous()
        hs, cs, gates_tm, cs_tm, hs_tm = k.clstm_scan_fwd_train(xs, h0c, c0c, w_ohwi, _f32(b))
        ctx.pack = pack
        ctx.params = (w, b)
        ctx.has_0 = (h0 is not None, c0 is not None)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xs, h0c, c0c, gates_tm, cs_tm, hs_tm, w_ihwo)
        return hs, cs

    @staticmethod
    def backward(ctx, dhs, dcs):
        k = default_kernels()
        xs, h0, c0, gates_tm, cs_tm, hs_tm, w_ihwo = ctx.saved_tensors
        w, b = ctx.params
        need = ctx.needs_input_grad
        tm = lambda d: None if d is None else d.float().transpose(0, 1).contiguous()
        dhs_tm = tm(dhs) if dhs is not None else torch.zeros_like(hs_tm)
        want_d0 = bool((ctx.has_0[0] and need[3]) or (ctx.has_0[1] and need[4]))
        dpre, dxs_tm, dh0, dc0 = k.clstm_scan_bwd(dhs_tm, tm(dcs), gates_tm, cs_tm, c0, w_ihwo, want_d0)
        dxs = dxs_tm.transpose(0, 1).contiguous() if need[0] else None
        dw, db = _bank_grads(k, xs.transpose(0, 1), h0, hs_tm, dpre, w, b, ctx.pack, need[1], need[2])
        return (dxs, dw, db, dh0 if ctx.has_0[0] and need[3] else None, dc0 if ctx.has_0[1] and need[4] else None, None)


class CLSTMGatesFn(torch.autograd.Function):
    """(h', c') = CLSTMCell's gate math on the gate convolution's output [.., 4C] and c [.., C] (common.py:376-385), one frame:
    the per-frame counterpart of CLSTMScanFn (kernels.clstm_gates_{fwd,bwd}, any format)."""

    @staticmethod
    def forward(ctx, gates, c_prev):
        gates, c_prev = gates.contiguous(), c_prev.contiguous()
        h, c = default_kernels().clstm_gates_fwd(gates, c_prev)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(gates, c_prev)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        gates, c_prev = ctx.saved_tensors
        dh = torch.zeros_like(c_prev) if dh is None else dh.contiguous()
        dgates, dc_prev = default_kernels().clstm_gates_bwd(dh, None if dc is None else dc.contiguous(), gates, c_prev)
        return dgates, dc_prev


# The three cell kinds: each holds its parameters under the reference's sub-module names (state_dict keys) and answers
#   step(conv, x, state, prefix, P, live)  one frame: x [B,5,8,C], previous state or None -> (features, new state); `conv` is
#                                          RefineNet._conv, P its packs, prefix the cell's name in them, live its CLSTM switch
#   scan(xs, init, prefix, P, live)        one clip: xs [B,T,5,8,C] -> (stacked state(s) [B,T,5,8,C], features for the next cell)
#   state_dtypes(scanned, dt)              the dtype(s) the state is carried in for compute dtype dt
#   SLOW_16BIT_SCAN_AT_128                 its bf16 / fp16 scan at C = 128 measured slower than the per-frame kernels

class CRNNCell(nn.Module):       # common.py:331-352
    SLOW_16BIT_SCAN_AT_128 = False

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.cell = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size=3, padding=1)

    def step(self, conv, x, state, prefix, P, live=False):
        h = torch.zeros_like(x) if state is None else state
        hnew = conv(torch.cat([x, h], dim=-1), prefix + '.cell', self.cell, P, act=ACT_TANH)
        return hnew, hnew

    def scan(self, xs, init, prefix, P, live=False):
        hs = CRNNScanFn.apply(xs.float(), self.cell.weight, self.cell.bias, init, P[prefix + '.cell'])
        return hs, hs.to(xs.dtype)

    def state_dtypes(self, scanned, dt):
        return torch.float32 if scanned else dt          # the float32 scan keeps its state in float32


class CLSTMCell(nn.Module):      # common.py:355-385
    SLOW_16BIT_SCAN_AT_128 = True

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.gates = nn.Conv2d(input_size + hidden_size, 4 * hidden_size, kernel_size=3, padding=1)

    def step(self, conv, x, state, prefix, P, live=False):
        h, c = (torch.zeros_like(x), torch.zeros_like(x)) if state is None else state
        if live:        # opt-in departure from the reference: h is the cell's output, gradients flow through it
            gates = conv(torch.cat([x, h], dim=-1), prefix + '.gates', self.gates, P)
            hn, cn = CLSTMGatesFn.apply(gates, c)
            return hn, (hn, cn)
        # state computed and stored, output dead (refine_net.py:168-174); forward-only kernels
        k = default_kernels()
        with torch.no_grad():
            gates = k.conv2d_fwd(torch.cat([x.detach(), h], dim=-1).contiguous(), P[prefix + '.gates'].ohwi, _f32(self.gates.bias), 1, 1)
            hn, cn = k.clstm_gates_fwd(gates, c.contiguous())
        return x, (hn, cn)

    def scan(self, xs, init, prefix, P, live=False):
        h_init, c_init = init if init is not None else (None, None)
        if live and torch.is_grad_enabled():      # h is the features: differentiable scan, h feeds on like CRNN's
            hcs = CLSTMScanFn.apply(xs.float(), self.gates.weight, self.gates.bias, h_init, c_init, P[prefix + '.gates'])
        else:           # dead, or inference (EVEStream, eval): the same hs / cs bit for bit, nothing kept for a backward
            hcs = clstm_scan(xs, self.gates.weight, self.gates.bias, P[prefix + '.gates'], h_init, c_init)
        return tuple(hcs), (hcs[0].to(xs.dtype) if live else xs)       # dead: every cell of a stack sees the bottleneck input

    def state_dtypes(self, scanned, dt):
        return (torch.float32, torch.float32) if scanned else (dt, dt)


class CGRUCell(nn.Module):       # common.py:388-415
    SLOW_16BIT_SCAN_AT_128 = True

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.gates_1 = nn.Conv2d(input_size + hidden_size, 2 * hidden_size, kernel_size=3, padding=1)
        self.gate_2 = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size=3, padding=1)

    def step(self, conv, x, state, prefix, P, live=False):
        h = torch.zeros_like(x) if state is None else state
        g1 = conv(torch.cat([x, h], dim=-1), prefix + '.gates_1', self.gates_1, P)
        ru, rh = CGRUGates1Fn.apply(g1, h)
        g2 = conv(torch.cat([rh, x], dim=-1), prefix + '.gate_2', self.gate_2, P)
        hnew = CGRUGates2Fn.apply(g2, ru, h)
        return hnew, hnew

    def scan(self, xs, init, prefix, P, live=False):
        hs = CGRUScanFn.apply(xs.contiguous(), self.gates_1.weight, self.gates_1.bias, self.gate_2.weight, self.gate_2.bias,
                              init, P[prefix + '.gates_1'], P[prefix + '.gate_2'])
        return hs, hs

    def state_dtypes(self, scanned, dt):
        return dt                                        # its scans run in the compute dtype (16-bit storage included)


def use_scan(cells, hwc, dtype):
    # the 5 x 8 x C bottleneck with C in SCAN_WIDTHS and any number of stacked cells: every cell takes the whole clip in ONE
    # persistent launch, cell i scanning cell i-1's states (which kernel per kind, width and format: DESIGN.md a10).  Every
    # other width stays on the per-frame loop, and so by default do CGRU and CLSTM in bf16 / fp16 at C = 128: their scans run
    # 4x the C = 64 arithmetic on the float32 MFMA and measured SLOWER than the per-frame 16-bit MFMA convolutions at
    # B = 32 x T = 30 (profiles/refine_scan_widths.md).  eve_dispatch_config.cgru_scan = 3 scans them too.
    cells, C = list(cells), tuple(hwc)[-1]
    flag = dispatch_flag(default_kernels(), 'cgru_scan', 1)
    if not (cells and tuple(hwc)[:2] == (5, 8) and C in SCAN_WIDTHS and dtype in HALF_DTYPES + (torch.float32,) and flag != 0):
        return False
    # stacks are homogeneous (Bottleneck builds them from one refine_net_rnn_type), so the first cell speaks for the stack
    slower = C == 128 and dtype in HALF_DTYPES and cells[0].SLOW_16BIT_SCAN_AT_128
    return flag == 3 or not slower
