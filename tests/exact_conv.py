"""Helpers of the bit-exact convolution tests (tests/test_gpu_conv_exact.py on the GPU, tests/test_conv_exact_host.py on the CPU).

Products of two 16-bit values are exact in float32.  With small-integer operands every partial sum is an integer below 2^24, so
float32 accumulation is exact in ANY order -- any tiling, split-K, atomics.  A correct kernel's result is then fully determined:
float32 outputs are the integer sum itself, 16-bit outputs that integer (+ integer bias, + the integer the tensor held before for the
accumulating entry points) rounded ONCE to nearest even.  The reference is torch's conv2d / conv_transpose2d / conv2d_weight on the CPU
in float64 (float32 for the big rows: equally exact below 2^24, and every row asserts that bound), then one `.to(dtype)`; the comparison
is `got == want` on every element.

Two operand regimes:
  exact     x from {-2, -1, 1, 2} ({-1, 1} beyond K = 1 152), w from {-1, 1}, bias from [-8, 8]: the sums are representable in the
            storage format as they stand (asserted: >= 99 % within 256 / 2 048), so a lost, doubled or misplaced term shows;
  rounding  x from +-{1..4}, w from +-{1..3}, bias / previous tensor of magnitude 300 .. 900 (float16: operands and bias scaled so
            that the sums pass 2 048): the one rounding is exercised, ties included (asserted: >= 2 % inexact, >= 1 % exact ties).
            An entry point with neither bias nor previous tensor and fewer than 576 terms gets larger x of mixed parity
            (plain_value_sets), so that its sums reach the rounding range by themselves; only the plain data gradient below
            K = 576 is excused, and only from the tie share.
"""
import contextlib
import ctypes

import torch
import torch.nn.functional as F

HALVES = (torch.bfloat16, torch.float16)
MANT = {torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.bfloat16: -126, torch.float16: -14}
EXACT_CAP = {torch.bfloat16: 256.0, torch.float16: 2048.0}      # integers up to here are representable
TNAME = {torch.bfloat16: 'eve::bf16_t', torch.float16: 'eve::f16_t', torch.float32: 'float'}
DT_ID = {torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float32: 'f32'}
GUARD_ROWS = 64
GUARD_VALUE = 7.0
LIMIT = float(1 << 24)
REF64_MAX_MACS = 1.5e9          # above: float32 reference (exact below 2^24, which every row asserts)



@contextlib.contextmanager
def reference_threads():
    """The CPU references run on at most 16 threads; the process's setting is put back afterwards."""
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    try:
        yield
    finally:
        torch.set_num_threads(old)


# ---------------------------------------------------------------------------------------------- operands
def pick(shape, values, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)].to(dtype)


def signed(mags):
    return [-m for m in mags] + list(mags)


def big_ints(shape, lo, hi, seed, dtype=torch.float32):
    """Integers of magnitude lo .. hi with random sign; in a 16-bit dtype: rounded to it, i.e. representable integers."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    s = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    return (m * s).to(dtype)


def value_sets(regime, dtype, K):
    """-> (x values, w values, (bias lo, bias hi)); K = depth of the product (taps x channels)."""
    if regime == 'exact':
        return (signed([1]) if K > 1152 else signed([1, 2])), signed([1]), (0, 8)
    assert regime == 'rounding'
    if dtype == torch.float16:
        # mixed parity and an rms of ~35: the sums of K >= 576 terms pass 2 048 and stay far below 65 504 (K = 4 608: std 5 300)
        return signed([13, 27, 38, 51]), signed([1, 2, 3]), (2400, 7200)
    return signed([1, 2, 3, 4]), signed([1, 2, 3]), (300, 900)


def plain_value_sets(regime, dtype, K, kmin=None):
    """value_sets for a product that nothing carries (no bias, no previous tensor).  Rounding regime below K = 576: x magnitudes
    {s, s + 1, 2 s + 1, 3 s + 2} (mixed parity, rms ~1.9 s) with s chosen so that the sums have a standard deviation of ~400 (bf16:
    the format rounds integers beyond 256) / ~3 000 (float16: beyond 2 048, and 65 504 stays ~20 deviations away)."""
    xv, wv, b = value_sets(regime, dtype, K)
    K = kmin or K                     # (the fewest terms any output sums: a strided data gradient's sparsest parity class)
    if regime == 'rounding' and K < 576:
        target = 3000.0 if dtype == torch.float16 else 400.0
        s = max(1, int(round(target / (2.16 * K ** 0.5 * 1.94))))
        xv = signed([s, s + 1, 2 * s + 1, 3 * s + 2])
    return xv, wv, b


def gen_bias(n, regime, dtype, K, seed):
    lo, hi = value_sets(regime, dtype, K)[2]
    if regime == 'exact':
        g = torch.Generator().manual_seed(seed)
        return torch.randint(-hi, hi + 1, (n,), generator=g).float()
    return big_ints((n,), lo, hi, seed)


def gen_prev(shape, regime, dtype, K, seed):
    """What an accumulating entry point finds in its output: integers representable in `dtype` (float32: any integer)."""
    lo, hi = value_sets(regime, dtype, K)[2]
    if regime == 'exact':
        g = torch.Generator().manual_seed(seed)
        return torch.randint(-hi, hi + 1, tuple(shape), generator=g).float().to(dtype)
    return big_ints(shape, lo, hi, seed, dtype)


# ---------------------------------------------------------------------------------------------- references (CPU)
def ref_dtype(macs):
    return torch.float64 if macs <= REF64_MAX_MACS else torch.float32


def nchw(t, rdt):
    return t.to(rdt).permute(0, 3, 1, 2)


def assert_below_2_24(bound, what):
    assert bound < LIMIT, '%s: sum of magnitudes may reach %.3g >= 2^24: float32 accumulation is no longer exact' % (what, bound)


def ref_fwd(x, w_ohwi, bias, stride, pad, what='fwd'):
    """x [N,H,W,Cin], w [Cout,KH,KW,Cin] (integer-valued, any dtype) -> float64 [N,OH,OW,Cout] = conv + bias, exact."""
    Cout, KH, KW, Cin = w_ohwi.shape
    amax = float(x.float().abs().max()) * float(w_ohwi.float().abs().max()) * KH * KW * Cin + (float(bias.abs().max()) if bias is not None else 0.0)
    assert_below_2_24(amax, what)
    OH, OW = (x.shape[1] + 2 * pad - KH) // stride + 1, (x.shape[2] + 2 * pad - KW) // stride + 1
    rdt = ref_dtype(float(x.shape[0]) * OH * OW * Cout * KH * KW * Cin)
    with reference_threads():
        y = F.conv2d(nchw(x, rdt), w_ohwi.to(rdt).permute(0, 3, 1, 2), None, stride, pad)
    y = y.permute(0, 2, 3, 1).double()
    return y + bias.double() if bias is not None else y


def ref_dgrad(dy, w_ihwo, in_hw, stride, pad, what='dgrad'):
    """dy [N,OH,OW,Cout], w [Cin,KH,KW,Cout] -> float64 [N,IH,IW,Cin]."""
    Cin, KH, KW, Cout = w_ihwo.shape
    assert_below_2_24(float(dy.float().abs().max()) * float(w_ihwo.float().abs().max()) * KH * KW * Cout, what)
    IH, IW = in_hw
    N, OH, OW, _ = dy.shape
    opad = (IH - ((OH - 1) * stride - 2 * pad + KH), IW - ((OW - 1) * stride - 2 * pad + KW))
    rdt = ref_dtype(float(N) * OH * OW * Cout * KH * KW * Cin)
    with reference_threads():
        dx = F.conv_transpose2d(nchw(dy, rdt), w_ihwo.to(rdt).permute(3, 0, 1, 2), None, stride, pad, output_padding=opad)
    assert tuple(dx.shape[2:]) == (IH, IW)
    return dx.permute(0, 2, 3, 1).double()


def ref_wgrad(x, dy, KH, KW, stride, pad, what='wgrad'):
    """-> float64 dw [Cout,KH,KW,Cin], db [Cout]; x here is the STAGED operand (after a prologue, if any)."""
    N, OH, OW, Cout = dy.shape
    Cin = x.shape[3]
    assert_below_2_24(float(x.float().abs().max()) * float(dy.float().abs().max()) * N * OH * OW, what)
    rdt = ref_dtype(float(N) * OH * OW * Cout * KH * KW * Cin)
    with reference_threads():
        dw = torch.nn.grad.conv2d_weight(nchw(x, rdt), (Cout, Cin, KH, KW), nchw(dy, rdt), stride, pad)
    return dw.permute(0, 2, 3, 1).double(), dy.double().sum(dim=(0, 1, 2))


def prologue(x, ss, pro_act, dtype):
    """The staged operand of the InstanceNorm prologue: act(x * scale + shift) per (image, channel), in the compute dtype."""
    z = x.double() * ss[:, None, None, :, 0].double() + ss[:, None, None, :, 1].double()
    if pro_act == 1:
        z = z.clamp(min=0)
    out = z.to(dtype)
    assert torch.equal(out.double(), z), 'the staged operand must be exact in the compute dtype'
    return out


def gen_scale_shift(N, C, seed):
    return torch.stack([pick((N, C), [0.5, 1.0, 2.0], seed), pick((N, C), [-1.0, 0.0, 1.0], seed + 1)], -1).contiguous()


def round_once(want64, dtype):
    """float64 -> storage format, nearest even, ONE rounding (the values are exact in float32, so the stop there is harmless)."""
    assert torch.equal(want64.float().double(), want64)
    return want64.float().to(dtype)


# ---------------------------------------------------------------------------------------------- conditions on the inputs
def ulp_storage(v64, dtype):
    """Spacing of the 16-bit format at |v| (float64 tensor)."""
    _, e = torch.frexp(v64.abs())
    e = torch.where(v64 == 0, torch.full_like(e, EMIN[dtype]), e - 1).clamp(min=EMIN[dtype])
    return torch.ldexp(torch.ones_like(v64), e - MANT[dtype])


def shares(want64, dtype):
    """-> (share within the exactly representable range, share inexact in `dtype`, share that are exact ties)."""
    r = want64.float().to(dtype).double()
    inexact = r != want64
    tie = (r - want64).abs() * 2 == ulp_storage(want64, dtype)
    return (float((want64.abs() <= EXACT_CAP[dtype]).double().mean()), float(inexact.double().mean()), float((inexact & tie).double().mean()))


def check_regime(want64, dtype, regime, what, ties_required=True):
    """The two conditions on the INPUTS, met by the reference alone.  ties_required = False: the plain data gradient below K = 576,
    which is excused from the tie share (not from the inexact share) of the rounding regime."""
    if dtype == torch.float32:
        return
    small, inexact, ties = shares(want64, dtype)
    print('%-40s %-8s within cap %.4f  inexact %.4f  ties %.4f%s' % (what, regime, small, inexact, ties, '' if ties_required else '  (tie share not required)'))
    if regime == 'exact':
        assert small >= 0.99, '%s: only %.4f of the reference outputs are representable integers' % (what, small)
    else:
        assert inexact >= 0.02 and (ties >= 0.01 or not ties_required), \
            '%s: the rounding regime rounds %.4f and ties %.4f of the outputs' % (what, inexact, ties)
        if dtype == torch.float16:
            assert float(want64.abs().max()) < 65504.0, '%s: the reference leaves the float16 range' % what


# ---------------------------------------------------------------------------------------------- the checker
def check_exact(got, want, what, names='nhwc'):
    """got == want on every element (values: -0 equals +0); a failure lists the first mismatching coordinates with both values."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    assert g.shape == w.shape, '%s: shape %s vs %s' % (what, tuple(g.shape), tuple(w.shape))
    assert bool(torch.isfinite(g).all()), '%s: non-finite values' % what
    bad = (g != w).nonzero()
    if bad.shape[0]:
        lines = ['(%s) = %s: got %r want %r' % (', '.join(names[:g.dim()]), tuple(int(i) for i in idx), float(g[tuple(idx)]), float(w[tuple(idx)]))
                 for idx in bad[:8]]
        raise AssertionError('%s: %d of %d elements differ, max |diff| %g\n  %s' % (what, bad.shape[0], g.numel(), float((g - w).abs().max()),
                                                                                  '\n  '.join(lines)))


def guarded(shape, dtype, device):
    """-> (buffer, view of `shape`): a tensor followed by a guard plane of 64 rows that nothing may write."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD_ROWS * shape[-1],), GUARD_VALUE, dtype=dtype, device=device)
    return buf, buf[:n].view(*shape)


def check_guard(buf, view, what):
    assert bool((buf[view.numel():] == GUARD_VALUE).all()), '%s: the guard plane behind the output was written' % what


# ---------------------------------------------------------------------------------------------- the two back ends
class HipCalls(object):
    """The C ABI with caller-owned outputs (so that a guard plane can sit behind them).  HipKernels allocates the outputs of most
    entry points itself, so this goes through its private helpers -- _desc (the eve_conv_desc), _p (checked device pointer), _ck (status
    -> exception), _stream, workspace -- and the argument order of include/eve_hip.h: a change to either has to be followed here."""

    def __init__(self, hip):
        self.hip = hip
        self.device = 'cuda'

    def last(self):
        return self.hip.lib.eve_last_kernel().decode()

    def override(self, **fields):
        return self.hip.dispatch_override(**fields) if fields else contextlib.nullcontext()

    def fwd(self, x, w, bias, stride, pad, act, y, acc=False, ss=None, pro_act=0):
        h = self.hip
        N, IH, IW, Cin = x.shape
        Cout, KH, KW, _ = w.shape
        d = h._desc(x.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        assert tuple(y.shape) == (N, d.OH, d.OW, Cout)
        h._ck(h.lib.eve_conv2d_fwd(ctypes.byref(d), h._p(x), h._p(w), h._p(bias), act | (0x100 if acc else 0), h._p(ss), pro_act, h._p(y),
                                   h._stream()))

    def fwd_stats(self, x, w, bias, stride, pad, act, y, mr):
        """-> whether the statistics were written"""
        h = self.hip
        N, IH, IW, Cin = x.shape
        Cout, KH, KW, _ = w.shape
        d = h._desc(x.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        written = ctypes.c_int(0)
        h._ck(h.lib.eve_conv2d_fwd_stats(ctypes.byref(d), h._p(x), h._p(w), h._p(bias), act, h._p(y), h._p(mr), 1e-5, ctypes.byref(written),
                                         h._stream()))
        return bool(written.value)

    def dgrad(self, dy, w_ihwo, stride, pad, dx, acc=False):
        h = self.hip
        N, IH, IW, Cin = dx.shape
        _, KH, KW, Cout = w_ihwo.shape
        d = h._desc(dy.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        assert tuple(dy.shape) == (N, d.OH, d.OW, Cout)
        if acc:
            h._ck(h.lib.eve_conv2d_dgrad_acc(ctypes.byref(d), h._p(dy), h._p(w_ihwo), h._p(dx), h._stream()))
        else:
            wsp, wsn = h.workspace(dy.device) if dy.dtype in HALVES else (None, 0)
            h._ck(h.lib.eve_conv2d_dgrad(ctypes.byref(d), h._p(dy), h._p(w_ihwo), h._p(dx), wsp, wsn, h._stream()))

    def wgrad(self, x, dy, KH, KW, stride, pad, dw, db=None, ss=None, pro_act=0, workspace=True):
        h = self.hip
        N, IH, IW, Cin = x.shape
        Cout = dy.shape[3]
        d = h._desc(x.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        wsp, wsn = h.workspace(x.device) if (workspace and x.dtype in HALVES) else (None, 0)
        if db is not None:
            h._ck(h.lib.eve_conv2d_wgrad_bias(ctypes.byref(d), h._p(x), h._p(dy), h._p(dw), h._p(db), wsp, wsn, h._stream()))
        else:
            h._ck(h.lib.eve_conv2d_wgrad(ctypes.byref(d), h._p(x), h._p(dy), h._p(ss), pro_act, h._p(dw), wsp, wsn, h._stream()))

    def bias_grad(self, dy, db):
        self.hip.bias_grad(dy, db)


class FakeCalls(object):
    """The same calls on tests/fake_kernels.FakeKernels (CPU ATen): what the CPU suite runs the checker on."""

    def __init__(self, fake):
        self.fake = fake
        self.device = 'cpu'

    def last(self):
        return None

    def override(self, **fields):
        return contextlib.nullcontext()

    def fwd(self, x, w, bias, stride, pad, act, y, acc=False, ss=None, pro_act=0):
        if acc:
            self.fake.conv2d_fwd(x, w, bias, stride, pad, act, accumulate_into=y)
        else:
            y.copy_(self.fake.conv2d_fwd(x, w, bias, stride, pad, act, ss=ss, pro_act=pro_act))

    def dgrad(self, dy, w_ihwo, stride, pad, dx, acc=False):
        if acc:
            self.fake.conv2d_dgrad(dy, w_ihwo, tuple(dx.shape[1:3]), stride, pad, accumulate_into=dx)
        else:
            dx.copy_(self.fake.conv2d_dgrad(dy, w_ihwo, tuple(dx.shape[1:3]), stride, pad))

    def wgrad(self, x, dy, KH, KW, stride, pad, dw, db=None, ss=None, pro_act=0, workspace=True):
        self.fake.conv2d_wgrad(x, dy, KH, KW, stride, pad, dw, ss=ss, pro_act=pro_act, db=db)

    def bias_grad(self, dy, db):
        self.fake.bias_grad(dy, db)


# ---------------------------------------------------------------------------------------------- one row
def kname(pattern, dtype):
    return pattern.replace('{T}', TNAME[dtype])


def launch_twice(calls, what, expect, dtype, shape, out_dtype, prev, fn):
    """Run `fn(out)` on two guarded outputs (each starting from `prev`, or from the guard value): the kernel that ran is `expect`,
    the guard planes keep their value, both results are equal.  -> the first result."""
    outs = []
    for _ in range(2):
        buf, view = guarded(shape, out_dtype, calls.device)
        if prev is not None:
            view.copy_(prev.to(calls.device))
        fn(view)
        used = calls.last()
        if used is not None and expect is not None:
            assert used == kname(expect, dtype), '%s ran on %s, expected %s' % (what, used, kname(expect, dtype))
        check_guard(buf, view, what)
        outs.append(view)
    assert torch.equal(outs[0], outs[1]), '%s: the same launch twice gives different results' % what
    return outs[0]


def run_conv_row(calls, row, dtype, regime):
    """Forward / data-gradient entry points of one table row (see CONV_ROWS in tests/test_gpu_conv_exact.py)."""
    N, H, W, Cin, Cout, ks, stride, pad = row['shape']
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    Kf, Kd = ks * ks * Cin, ks * ks * Cout
    dev = calls.device
    tag = '%s %s ' % (row['id'], DT_ID[dtype])
    ops = row['ops']
    with calls.override(**row.get('override', {})):
        if any(o.startswith('fwd') for o in ops):
            # (a row whose forward has no bias -- the strided shortcut -- has nothing else to carry its sums: larger operands)
            xv, wv, _ = (plain_value_sets if 'fwd_nobias' in ops else value_sets)(regime, dtype, Kf)
            x, w = pick((N, H, W, Cin), xv, 1, dtype), pick((Cout, ks, ks, Cin), wv, 2, dtype)
            bias = gen_bias(Cout, regime, dtype, Kf, 3)
            xd, wd, bd = x.to(dev), w.to(dev), bias.to(dev)
            yshape = (N, OH, OW, Cout)
            plain = ref_fwd(x, w, None, stride, pad, tag + 'fwd') if any(o in ops for o in ('fwd', 'fwd_relu', 'fwd_nobias', 'fwd_acc')) else None
            for op in ('fwd', 'fwd_relu', 'fwd_nobias', 'fwd_acc'):
                if op not in ops:
                    continue
                b = None if op == 'fwd_nobias' else bias
                want = plain if b is None else plain + b.double()
                assert_below_2_24(float(want.abs().max()), tag + op)
                prev = None
                if op == 'fwd_relu':
                    want = want.clamp(min=0)
                if op == 'fwd_acc':
                    prev = gen_prev(yshape, regime, dtype, Kf, 4)
                    want = want + prev.double()
                    assert_below_2_24(float(want.abs().max()), tag + op)
                check_regime(want, dtype, regime, tag + op)
                got = launch_twice(calls, tag + op, ops[op], dtype, yshape, dtype, prev,
                                   lambda y: calls.fwd(xd, wd, None if b is None else bd, stride, pad, 1 if op == 'fwd_relu' else 0, y,
                                                       acc=(op == 'fwd_acc')))
                check_exact(got, round_once(want, dtype), tag + op)
            for pro_act, op in ((0, 'fwd_ss'), (1, 'fwd_ss_relu')):
                if op not in ops:
                    continue
                ss = gen_scale_shift(N, Cin, 5)
                want = ref_fwd(prologue(x, ss, pro_act, dtype), w, bias, stride, pad, tag + op)
                check_regime(want, dtype, regime, tag + op)
                ssd = ss.to(dev)
                got = launch_twice(calls, tag + op, ops[op], dtype, yshape, dtype, None,
                                   lambda y: calls.fwd(xd, wd, bd, stride, pad, 0, y, ss=ssd, pro_act=pro_act))
                check_exact(got, round_once(want, dtype), tag + op)
        if any(o.startswith('dgrad') for o in ops):
            # (a strided data gradient sums only the taps of its parity class: a ninth of them at the least)
            kmin = Kd // 9 if (stride == 2 and ks == 3) else Kd
            xv, wv, _ = plain_value_sets(regime, dtype, Kd, kmin) if 'dgrad' in ops else value_sets(regime, dtype, Kd)
            dy = pick((N, OH, OW, Cout), xv, 6, dtype)
            w_ihwo = pick((Cin, ks, ks, Cout), wv, 7, dtype)
            dyd, wtd = dy.to(dev), w_ihwo.to(dev)
            want = ref_dgrad(dy, w_ihwo, (H, W), stride, pad, tag + 'dgrad')
            if 'dgrad' in ops:
                check_regime(want, dtype, regime, tag + 'dgrad', ties_required=kmin >= 576)
                got = launch_twice(calls, tag + 'dgrad', ops['dgrad'], dtype, (N, H, W, Cin), dtype, None,
                                   lambda dx: calls.dgrad(dyd, wtd, stride, pad, dx))
                check_exact(got, round_once(want, dtype), tag + 'dgrad')
            if 'dgrad_acc' in ops:
                prev = gen_prev((N, H, W, Cin), regime, dtype, Kd, 8)
                want_acc = want + prev.double()
                assert_below_2_24(float(want_acc.abs().max()), tag + 'dgrad_acc')
                check_regime(want_acc, dtype, regime, tag + 'dgrad_acc')
                got = launch_twice(calls, tag + 'dgrad_acc', ops['dgrad_acc'], dtype, (N, H, W, Cin), dtype, prev,
                                   lambda dx: calls.dgrad(dyd, wtd, stride, pad, dx, acc=True))
                check_exact(got, round_once(want_acc, dtype), tag + 'dgrad_acc')


def run_wgrad_row(calls, row, dtype, regime):
    """Weight-gradient entry points of one table row, accumulating onto integer-valued dw0 / db0: float32 outputs, exact integers."""
    N, H, W, Cin, Cout, ks, stride, pad = row['shape']
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    dev = calls.device
    tag = '%s %s ' % (row['id'], DT_ID[dtype])
    ops = row['ops']
    xv, wv, _ = value_sets(regime, torch.bfloat16, 1)          # (float32 outputs: the bf16 value sets serve every dtype)
    x, dy = pick((N, H, W, Cin), xv, 11, dtype), pick((N, OH, OW, Cout), wv, 12, dtype)
    dw0, db0 = big_ints((Cout, ks, ks, Cin), 300, 900, 13), big_ints((Cout,), 300, 900, 14)
    xd, dyd = x.to(dev), dy.to(dev)
    names = ('o', 'kh', 'kw', 'i')
    with calls.override(**row.get('override', {})):
        want_dw, want_db = None, None
        for op in ('wgrad', 'wgrad_bias', 'wgrad_nows', 'wgrad_ss', 'wgrad_ss_relu'):
            if op not in ops:
                continue
            ss, xin = None, x
            pro_act = 1 if op == 'wgrad_ss_relu' else 0
            if op.startswith('wgrad_ss'):
                ss = gen_scale_shift(N, Cin, 15)
                xin = prologue(x, ss, pro_act, dtype)
            if want_dw is None or ss is not None:
                ref_dw, ref_db = ref_wgrad(xin, dy, ks, ks, stride, pad, tag + op)
                if ss is None:
                    want_dw, want_db = ref_dw, ref_db
            else:
                ref_dw, ref_db = want_dw, want_db
            assert_below_2_24(float((ref_dw.abs() + dw0.double().abs()).max()), tag + op)
            ssd = None if ss is None else ss.to(dev)
            if op == 'wgrad_bias':
                both = torch.cat([dw0.reshape(-1), db0])       # one buffer: the guard plane sits behind db

                def fn(out):
                    n = dw0.numel()
                    calls.wgrad(xd, dyd, ks, ks, stride, pad, out[:n].view(Cout, ks, ks, Cin), db=out[n:])
                got = launch_twice(calls, tag + op, ops[op], dtype, (both.numel(),), torch.float32, both, fn)
                check_exact(got[:dw0.numel()].view(Cout, ks, ks, Cin), ref_dw + dw0.double(), tag + op + ' dw', names)
                check_exact(got[dw0.numel():], ref_db + db0.double(), tag + op + ' db', ('o',))
            else:
                got = launch_twice(calls, tag + op, ops[op], dtype, (Cout, ks, ks, Cin), torch.float32, dw0,
                                   lambda dw: calls.wgrad(xd, dyd, ks, ks, stride, pad, dw, ss=ssd, pro_act=pro_act,
                                                          workspace=(op != 'wgrad_nows')))
                check_exact(got, ref_dw + dw0.double(), tag + op, names)
        if 'bias_grad' in ops:
            got = launch_twice(calls, tag + 'bias_grad', None, dtype, (Cout,), torch.float32, db0, lambda db: calls.bias_grad(dyd, db))
            check_exact(got, dy.double().sum(dim=(0, 1, 2)) + db0.double(), tag + 'bias_grad', ('o',))
