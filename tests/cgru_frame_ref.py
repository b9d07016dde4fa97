"""The teacher-forced float64 reference of the 16-bit conv-GRU clip scans and its judge; shared by test_cgru_frame_ref_host.py
(the judge against right and deliberately wrong stand-ins) and test_gpu_cgru_scan_frames.py (the six kernels).  CPU only.

Every stored tensor of a scan is judged frame by frame against float64 evaluated on the tensors the scan ITSELF stored (the
previous state, the rounded gates, r * h, the rounded pre-activation gradients), so no rounding decision of one frame is amplified
by the frames after it and each element can be held to half a unit of the storage format:

    |got - v64| <= 1/2 ulp_H(v64) + eps,     eps = margin * max |v32 - v64| over that tensor and frame (>= 2^-22 max |v64|)

v32 is the same frame in float32 (ATen, same stored operands, the float64 backward carry cast to float): eps is measured on the
reference, never on the code under test.  margin = 8 covers what one CPU summation order does not show: the MFMA order of K = 576 /
1 152 / 2 304 products, the hardware exponential and reciprocal of sigmoid_rcp / tanh_rcp, the float32 carry over T frames.
Two caps keep the inputs honest: at most 1 % of a tensor's elements may differ from RNE_H(v64) at all, and at most 1 % may lie
below the format's smallest normal (those are judged with that smallest normal as an absolute tolerance: flushed or kept)."""
import torch

import refine_variants as rv

MARGIN = 8
FORMATS = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}        # significand bits (hidden one included), exponent of the smallest normal
CAP = 0.01
SHAPES = [(1, 1, False), (4, 2, True), (5, 3, False), (7, 30, True)]       # (B, T, with h0) of the forward and backward cases
WIDTHS = (32, 64, 128)


def seed_of(C, B, T):
    return 1000 * C + 10 * B + T


def ulp(v64, dt):
    """Spacing of format dt at |v64| (the wider binade's at a power of two), floored at the spacing of the smallest normal."""
    p, emin = FORMATS[dt]
    e = torch.frexp(v64.abs())[1] - 1                                    # floor(log2 |v|), exactly
    e = torch.where(v64 == 0, torch.full_like(e, emin), e)
    return torch.ldexp(torch.ones_like(v64), e.clamp_min(emin) - (p - 1))


def rne(v, dt):
    """v rounded to nearest-even in dt, returned in v's dtype."""
    return v.to(dt).to(v.dtype)


def truncate(v, dt):
    """v (float32) rounded TOWARDS ZERO to dt, as float32: the wrong rounding of the host self-test."""
    h = v.to(dt)
    bits = h.view(torch.int16)
    return torch.where(h.float().abs() > v.abs(), bits - 1, bits).view(dt).float()


def make_inputs(C, B, T, with_h0, dt, seed, gain=1.0):
    """The operands of the GPU cases (scales of test_gpu_refine_scan_variants.py), 16-bit valued CPU tensors of dtype dt; biases
    float32.  Forward: xs, h0, w1, b1, w2, b2.  Backward, synthetic as in test_fused_cgru_scan_backward_kernel_matches_contract: dhs,
    ru, og, hs_tm and the IHWO banks w1t, w2t of the same filters."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape, scale=1.0: (torch.randn(shape, generator=g) * scale).to(dt)
    s = 0.04 * (64.0 / C) ** 0.5 * gain
    d = {'xs': rn(B, T, 5, 8, C, scale=0.8), 'h0': rn(B, 5, 8, C, scale=0.5),
         'w1': rn(2 * C, 3, 3, 2 * C, scale=s), 'w2': rn(C, 3, 3, 2 * C, scale=s),
         'b1': torch.randn(2 * C, generator=g) * 0.2, 'b2': torch.randn(C, generator=g) * 0.2,
         'dhs': rn(T, B, 5, 8, C),
         'ru': torch.sigmoid(torch.randn((T, B, 5, 8, 2 * C), generator=g)).to(dt),
         'og': torch.tanh(torch.randn((T, B, 5, 8, C), generator=g)).to(dt),
         'hs_tm': rn(T, B, 5, 8, C, scale=0.6)}
    if not with_h0:
        d['h0'] = None
    d['w1t'], d['w2t'] = d['w1'].permute(3, 1, 2, 0).contiguous(), d['w2'].permute(3, 1, 2, 0).contiguous()
    return d


class Report:
    """What the judge found: per tensor the worst (excess over 1/2 ulp) / max |v32 - v64|, the share of elements that differ
    from RNE_H(v64), the share below the smallest normal; `failures` is empty when everything holds."""

    def __init__(self, dt, margin, caps):
        self.dt, self.margin, self.caps = dt, margin, caps
        self.ratio, self.failures = {}, []
        self._flips, self._below, self._count = {}, {}, {}

    def flips(self, name):
        return self._flips[name] / self._count[name]

    def below(self, name):
        return self._below[name] / self._count[name]

    def judge(self, name, t, got, v64, v32):
        got = got.double()
        assert tuple(got.shape) == tuple(v64.shape) == tuple(v32.shape), name
        tiny = 2.0 ** FORMATS[self.dt][1]
        if not bool(torch.isfinite(got).all()):
            self.failures.append('%s[%s]: not finite' % (name, t))
        dev = max(float((v32.double() - v64).abs().max()), 2.0 ** -22 * float(v64.abs().max()) / self.margin, 1e-300)
        small = v64.abs() < tiny
        err = (got - v64).abs()
        excess = torch.where(small, err - tiny, err - 0.5 * ulp(v64, self.dt))
        ratio = float(torch.where(small, excess.clamp_max(0.0), excess).max()) / dev       # reported over the normal range
        self.ratio[name] = max(self.ratio.get(name, float('-inf')), ratio)
        bad = torch.where(small, excess > 0, excess > self.margin * dev)
        if bool(bad.any()):
            i = int(torch.where(bad, excess, torch.full_like(excess, float('-inf'))).argmax())
            where = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), got.shape))
            g, v, x = (float(a.flatten()[i]) for a in (got, v64, excess))
            self.failures.append('%s[%s]: %d of %d outside 1/2 ulp + %d x %.2e; worst at %s: got %.9g, float64 %.9g, excess %.3e = %.1f x'
                                 % (name, t, int(bad.sum()), bad.numel(), self.margin, dev, where, g, v, x, x / dev))
        self._flips[name] = self._flips.get(name, 0) + int((got != rne(v64, self.dt)).sum())
        self._below[name] = self._below.get(name, 0) + int((small & (v64 != 0)).sum())     # an exact zero (a zero state's r * h) is no underflow
        self._count[name] = self._count.get(name, 0) + got.numel()

    def exact(self, name, t, got, want):
        n = int((got != want).sum()) if got.shape == want.shape else -1
        if n:
            self.failures.append('%s[%s]: %d of %d elements are not bit-identical' % (name, t, n, want.numel()))

    def close(self):
        if self.caps:
            for name in self._count:
                if self.flips(name) > CAP:
                    self.failures.append('%s: %.3f %% of the elements differ from RNE(float64), cap 1 %%' % (name, 100 * self.flips(name)))
                if self.below(name) > CAP:
                    self.failures.append('%s: %.3f %% of the reference lies below the smallest normal, cap 1 %%' % (name, 100 * self.below(name)))
        return self

    @property
    def ok(self):
        return not self.failures

    def summary(self):
        return ', '.join('%s %.2f (differs %.3f%%, subnormal %.3f%%)' % (n, self.ratio[n], 100 * self.flips(n), 100 * self.below(n))
                         for n in self.ratio)

    def assert_ok(self, what=''):
        assert self.ok, '%s: %d findings, first: %s' % (what, len(self.failures), ' | '.join(self.failures[:4]))


def judge_forward(dt, xs, h0, w1, b1, w2, b2, hs, hs_tm, ru, rh, og, margin=MARGIN, caps=True):
    """The five tensors a forward scan stored against the teacher-forced float64 frame.  Operands and outputs: CPU tensors of dtype
    dt (biases float32), layouts of eve_cgru_scan_fwd."""
    B, T, C = xs.shape[0], xs.shape[1], xs.shape[-1]
    rep = Report(dt, margin, caps)
    for name, t_, shape in (('hs', hs, (B, T, 5, 8, C)), ('hs_tm', hs_tm, (T, B, 5, 8, C)), ('ru', ru, (T, B, 5, 8, 2 * C)),
                            ('rh', rh, (T, B, 5, 8, C)), ('og', og, (T, B, 5, 8, C))):
        assert t_.dtype == dt and tuple(t_.shape) == shape, (name, t_.dtype, tuple(t_.shape))
    first = (torch.zeros_like(hs_tm[0]) if h0 is None else h0)[None]
    hp16 = torch.cat([first, hs_tm[:-1]], 0)                                # h_{t-1} as stored, time-major
    x_tm = xs.transpose(0, 1)
    want = {}
    for f in (torch.float64, torch.float32):
        x, hp, r, u, o = x_tm.to(f), hp16.to(f), ru[..., :C].to(f), ru[..., C:].to(f), og.to(f)
        pre1 = rv._conv(torch.cat([x, hp], -1).flatten(0, 1), w1.to(f), b1.to(f)).unflatten(0, (T, B))
        pre2 = rv._conv(torch.cat([rh.to(f), x], -1).flatten(0, 1), w2.to(f), b2.to(f)).unflatten(0, (T, B))
        want[f] = {'ru': torch.sigmoid(pre1), 'og': torch.tanh(pre2), 'hs_tm': (1 - u) * o + u * hp}
    for t in range(T):
        for name, got in (('ru', ru), ('og', og), ('hs_tm', hs_tm)):
            rep.judge(name, t, got[t], want[torch.float64][name][t], want[torch.float32][name][t])
        # two stored 16-bit values multiplied in float32 are exact: one rounding, no allowance
        rep.exact('rh', t, rh[t], (ru[t][..., :C].float() * hp16[t].float()).to(dt))
    rep.exact('hs', 'all', hs, hs_tm.transpose(0, 1))
    return rep.close()


def judge_backward(dt, dhs, ru, og, hs_tm, h0, w1t, w2t, dg1, dg2, dxs, dh0, margin=MARGIN, caps=True):
    """The tensors a backward scan stored against the float64 frame, teacher-forced through the stored dg2_all / dg1_all (what
    the kernels hand to their data-gradient GEMMs); the carry is the reference's own, in float64 over the whole clip.  dh0 None =
    not asked for."""
    T, B, C = dhs.shape[0], dhs.shape[1], dhs.shape[-1]
    rep = Report(dt, margin, caps)
    for name, t_, shape in (('dg1', dg1, (T, B, 5, 8, 2 * C)), ('dg2', dg2, (T, B, 5, 8, C)), ('dxs', dxs, (T, B, 5, 8, C))) + \
            ((('dh0', dh0, (B, 5, 8, C)),) if dh0 is not None else ()):
        assert t_.dtype == dt and tuple(t_.shape) == shape, (name, t_.dtype, tuple(t_.shape))
    first = (torch.zeros_like(hs_tm[0]) if h0 is None else h0)[None]
    hp16 = torch.cat([first, hs_tm[:-1]], 0)
    op = {}
    for f in (torch.float64, torch.float32):
        dcat2 = rv._dgrad(dg2.to(f).flatten(0, 1), w2t.to(f)).unflatten(0, (T, B))
        dcat1 = rv._dgrad(dg1.to(f).flatten(0, 1), w1t.to(f)).unflatten(0, (T, B))
        op[f] = (dhs.to(f), ru[..., :C].to(f), ru[..., C:].to(f), og.to(f), hp16.to(f), dcat2[..., :C], dcat2[..., C:], dcat1[..., :C], dcat1[..., C:])
    carry = torch.zeros((B, 5, 8, C), dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        v = {}
        for f in (torch.float64, torch.float32):
            d, r, u, o, hp, drh, dx2, dx1, dhc = (a[t] for a in op[f])
            dhn = d + carry.to(f)
            v[f] = {'dg2': dhn * (1 - u) * (1 - o * o), 'dg1': torch.cat([drh * hp * r * (1 - r), dhn * (hp - o) * u * (1 - u)], -1),
                    'dxs': dx1 + dx2, 'dh0': dhn * u + drh * r + dhc}
        carry = v[torch.float64]['dh0']
        for name, got in (('dg2', dg2), ('dg1', dg1), ('dxs', dxs)):
            rep.judge(name, t, got[t], v[torch.float64][name], v[torch.float32][name])
        if t == 0 and dh0 is not None:
            rep.judge('dh0', 0, dh0, v[torch.float64]['dh0'], v[torch.float32]['dh0'])
    return rep.close()
