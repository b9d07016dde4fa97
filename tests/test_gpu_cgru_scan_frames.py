"""GPU: the six 16-bit conv-GRU clip scans -- cgru_scan_{fwd,bwd}_kernel (three sequences per workgroup), cgru_scan1_{fwd,bwd}_kernel
(one per workgroup), cgru_scan_f32_{fwd,bwd}_kernel<C, H> (16-bit storage on the float32 MFMA, C = 32 and 128) -- in bf16 AND f16, frame
by frame against the teacher-forced float64 reference of cgru_frame_ref.py: every stored element within half a unit of the format
plus 8 x the float32-vs-float64 deviation of the reference itself, r * h and the two layouts of the state bit for bit.  Plus: saturated
gates, sequences independent of their workgroup neighbours bit for bit, and nothing written outside the outputs.  The CPU side (the
judge against right and wrong stand-ins, at these inputs): test_cgru_frame_ref_host.py.

Measured on an MI355X, the margin at 8: per family and format the worst (excess over 1/2 ulp) / max |v32 - v64| over every case below
(the saturated ones included; 8 is the limit, 0.00 = never outside half a unit), then the largest share of a tensor that differs
from RNE(float64) at all and the largest share of the reference below the smallest normal (caps: 1 %; unsaturated cases):
    three-per-workgroup  bf16  ru 0.16  og 0.26  hs_tm 0.00  dg2 0.63  dg1 0.25  dxs 0.66  dh0 0.20   differs 0.039 %  subnormal 0
    three-per-workgroup  f16   ru 0.21  og 0.30  hs_tm 0.50  dg2 0.35  dg1 0.55  dxs 0.47  dh0 0.42   differs 0.117 %  subnormal 0.518 %
    one-per-workgroup    bf16  ru 0.38  og 0.25  hs_tm 0.00  dg2 0.29  dg1 0.32  dxs 0.37  dh0 0.09   differs 0.039 %  subnormal 0
    one-per-workgroup    f16   ru 0.25  og 0.18  hs_tm 0.50  dg2 0.58  dg1 0.45  dxs 0.51  dh0 0.28   differs 0.156 %  subnormal 0.516 %
    f32-mfma-c32         bf16  ru 0.09  og 0.22  hs_tm 0.00  dg2 0.28  dg1 0.23  dxs 0.34  dh0 0.50   differs 0.078 %  subnormal 0
    f32-mfma-c32         f16   ru 0.30  og 0.43  hs_tm 0.25  dg2 0.47  dg1 0.58  dxs 0.63  dh0 0.36   differs 0.234 %  subnormal 0.527 %
    f32-mfma-c128        bf16  ru 0.46  og 0.66  hs_tm 0.00  dg2 0.95  dg1 0.71  dxs 2.65  dh0 0.89   differs 0.037 %  subnormal 0
    f32-mfma-c128        f16   ru 0.57  og 0.90  hs_tm 0.25  dg2 1.65  dg1 2.83  dxs 2.65  dh0 1.71   differs 0.417 %  subnormal 0.524 %
r * h, hs against hs_tm, the independence and the guard bands: exact everywhere.  f16 subnormals are kept by all six kernels (the
saturated f16 gates, 7.8 % of them subnormal, differ from RNE(float64) in 0.19 % of the elements at most).
"""
import functools

import pytest
import torch

import cgru_frame_ref as cf
from eve_amd.kernels import default_kernels, dt_code

pytestmark = pytest.mark.gpu

# family: (width, dispatch override, kernel name with the direction and the format left open)
FAMILIES = {
    'three-per-workgroup': (64, dict(cgru_seq_max_b=0), 'cgru_scan_%s_kernel<eve::%s>'),
    'one-per-workgroup': (64, dict(cgru_seq_max_b=384), 'cgru_scan1_%s_kernel<eve::%s>'),
    'f32-mfma-c32': (32, {}, 'cgru_scan_f32_%s_kernel<32, eve::%s>'),
    'f32-mfma-c128': (128, {}, 'cgru_scan_f32_%s_kernel<128, eve::%s>'),
}
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}
both = lambda f: pytest.mark.parametrize('fmt', sorted(DTYPES))(pytest.mark.parametrize('family', sorted(FAMILIES))(f))
shape_id = lambda s: 'B%d-T%d-%s' % (s[0], s[1], 'h0' if s[2] else 'zero-state')
cu = lambda t: None if t is None else t.cuda()


@functools.lru_cache(maxsize=None)
def inputs(C, B, T, with_h0, fmt, saturated=False):
    """The operands the host file judges its stand-ins on (read only: shared between cases)."""
    if saturated:
        return cf.make_inputs(C, B, T, with_h0, DTYPES[fmt], cf.seed_of(C, B, T) + 1, gain=8.0)
    return cf.make_inputs(C, B, T, with_h0, DTYPES[fmt], cf.seed_of(C, B, T))


def forward(family, fmt, inp):
    """-> (hs, hs_tm, ru, rh, og) on the device, from the family's kernel in this format (asserted)."""
    hip = default_kernels()
    _, over, name = FAMILIES[family]
    with hip.dispatch_override(**over):
        got = hip.cgru_scan_fwd(cu(inp['xs']), cu(inp['h0']), cu(inp['w1']), cu(inp['b1']), cu(inp['w2']), cu(inp['b2']))
        assert hip.lib.eve_last_kernel().decode() == name % ('fwd', fmt + '_t')
    return got


def backward(family, fmt, inp):
    """-> (dg1, dg2, dxs, dh0 or None) on the device; dh0 is asked for where there is an h0."""
    hip = default_kernels()
    _, over, name = FAMILIES[family]
    with hip.dispatch_override(**over):
        got = hip.cgru_scan_bwd(cu(inp['dhs']), cu(inp['ru']), cu(inp['og']), cu(inp['hs_tm']), cu(inp['h0']), cu(inp['w1t']), cu(inp['w2t']),
                                want_dh0=inp['h0'] is not None)
        assert hip.lib.eve_last_kernel().decode() == name % ('bwd', fmt + '_t')
    return got


def judge_forward(inp, fmt, got, **kw):
    return cf.judge_forward(DTYPES[fmt], inp['xs'], inp['h0'], inp['w1'], inp['b1'], inp['w2'], inp['b2'], *[t.cpu() for t in got], **kw)


def judge_backward(inp, fmt, got, **kw):
    return cf.judge_backward(DTYPES[fmt], inp['dhs'], inp['ru'], inp['og'], inp['hs_tm'], inp['h0'], inp['w1t'], inp['w2t'],
                             *[None if t is None else t.cpu() for t in got], **kw)


# ------------------------------------------------------------------------------------------------ 1. frame by frame
@pytest.mark.parametrize('shape', cf.SHAPES, ids=shape_id)
@both
def test_forward_frames_within_half_a_unit_of_float64(family, fmt, shape):
    """(1, 1) and (4, 2), (5, 3): one and two live sequences in the last workgroup of the three-per-workgroup form; (7, 30): a
    whole clip through the filter ring and the software pipeline."""
    inp = inputs(FAMILIES[family][0], *shape, fmt)
    rep = judge_forward(inp, fmt, forward(family, fmt, inp))
    print('RATIO forward %s %s %s: %s' % (family, fmt, shape_id(shape), rep.summary()))
    rep.assert_ok('forward')


@pytest.mark.parametrize('shape', cf.SHAPES, ids=shape_id)
@both
def test_backward_frames_within_half_a_unit_of_float64(family, fmt, shape):
    """On synthetic ru / og / hs (as test_fused_cgru_scan_backward_kernel_matches_contract builds them); the whole clip also on the
    tensors the family's own forward stored."""
    inp = inputs(FAMILIES[family][0], *shape, fmt)
    rep = judge_backward(inp, fmt, backward(family, fmt, inp))
    print('RATIO backward %s %s %s: %s' % (family, fmt, shape_id(shape), rep.summary()))
    rep.assert_ok('backward')
    if shape[:2] == (7, 30):
        _, hs_tm, ru, _, og = forward(family, fmt, inp)
        own = dict(inp, hs_tm=hs_tm.cpu(), ru=ru.cpu(), og=og.cpu())
        rep = judge_backward(own, fmt, backward(family, fmt, own))
        print('RATIO backward-of-forward %s %s %s: %s' % (family, fmt, shape_id(shape), rep.summary()))
        rep.assert_ok('backward on the forward\'s tensors')


@both
def test_saturated_gates_stay_finite_and_within_the_bound(family, fmt):
    """Filters x 8: gates of exactly 1 and tanh gates of exactly +-1; sigmoid gates of exactly 0 in f16 (bf16 has float32's range:
    there they get below 2^-9, so their complement is exactly 1).  The bound is the same; the two caps on the inputs do not apply
    (a tenth of the f16 gates is subnormal by construction)."""
    inp = inputs(FAMILIES[family][0], 4, 2, True, fmt, saturated=True)
    got = forward(family, fmt, inp)
    ru, og = got[2].float().cpu(), got[4].float().cpu()
    assert bool((ru == 1).any()) and bool((og.abs() == 1).any()) and float(ru.min()) < 2.0 ** -9
    assert fmt != 'f16' or bool((ru == 0).any())
    rep = judge_forward(inp, fmt, got, caps=False)
    print('RATIO saturated-forward %s %s: %s' % (family, fmt, rep.summary()))
    rep.assert_ok('saturated forward')
    own = dict(inp, hs_tm=got[1].cpu(), ru=got[2].cpu(), og=got[4].cpu())
    rep = judge_backward(own, fmt, backward(family, fmt, own), caps=False)
    print('RATIO saturated-backward %s %s: %s' % (family, fmt, rep.summary()))
    rep.assert_ok('saturated backward')


# ------------------------------------------------------------------------------------------------ 2. independence
@both
def test_a_sequence_does_not_depend_on_its_neighbours(family, fmt):
    """Sequences 0, 1, 2 (one workgroup of the three-per-workgroup form) and 6 (alone in the last one) of a B = 7, T = 3 call equal a
    B = 1 call on that sequence alone, forward and backward, bit for bit."""
    inp = inputs(FAMILIES[family][0], 7, 3, True, fmt)
    fwd, bwd = forward(family, fmt, inp), backward(family, fmt, inp)
    batch_dim = {'xs': 0, 'h0': 0, 'dhs': 1, 'ru': 1, 'og': 1, 'hs_tm': 1}
    for s in (0, 1, 2, 6):
        one = {k: (v.narrow(batch_dim[k], s, 1).contiguous() if k in batch_dim else v) for k, v in inp.items()}
        for name, a, b in zip(('hs', 'hs_tm', 'ru', 'rh', 'og'), fwd, forward(family, fmt, one)):
            assert torch.equal(a.narrow(0 if name == 'hs' else 1, s, 1), b), (name, s)
        for name, a, b in zip(('dg1', 'dg2', 'dxs', 'dh0'), bwd, backward(family, fmt, one)):
            assert torch.equal(a.narrow(0 if name == 'dh0' else 1, s, 1), b), (name, s)


# ------------------------------------------------------------------------------------------------ 3. nothing outside the outputs
GUARD, SENTINEL = 4096, 0x5A5A              # elements on either side of an output (8 KiB: the 16-byte alignment is kept); their value


def guarded(shape, dt):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int16, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(dt).view(*shape)


def check_guards(bufs, what):
    for name, (buf, view) in bufs.items():
        n = view.numel()
        assert bool((buf[:GUARD] == SENTINEL).all()), '%s: written in front of %s' % (what, name)
        assert bool((buf[GUARD + n:] == SENTINEL).all()), '%s: written behind %s' % (what, name)


@pytest.mark.parametrize('B', [4, 5])
@both
def test_nothing_is_written_outside_the_outputs(family, fmt, B):
    """The entry points with caller-owned outputs, each a view inside a sentinel-filled buffer with a guard band on both sides:
    B = 4 and 5 leave the three-per-workgroup form one and two live sequences in its last workgroup.  The guards come back
    untouched and the outputs equal those of the allocating wrappers."""
    hip = default_kernels()
    C, over, name = FAMILIES[family]
    T, dt = 2, DTYPES[fmt]
    inp = inputs(C, B, T, True, fmt)
    d = {k: cu(v) for k, v in inp.items()}
    want_f, want_b = forward(family, fmt, inp), backward(family, fmt, inp)
    out_f = {n: guarded(s, dt) for n, s in (('hs', (B, T, 5, 8, C)), ('hs_tm', (T, B, 5, 8, C)), ('ru', (T, B, 5, 8, 2 * C)),
                                            ('rh', (T, B, 5, 8, C)), ('og', (T, B, 5, 8, C)))}
    out_b = {n: guarded(s, dt) for n, s in (('dg1', (T, B, 5, 8, 2 * C)), ('dg2', (T, B, 5, 8, C)), ('dxs', (T, B, 5, 8, C)),
                                            ('dh0', (B, 5, 8, C)))}
    p = hip._p
    with hip.dispatch_override(**over):
        hip._ck(hip.lib.eve_cgru_scan_fwd_c(dt_code(dt), B, T, C, p(d['xs']), p(d['h0']), p(d['w1']), p(d['b1']), p(d['w2']), p(d['b2']),
                                            *[p(out_f[n][1]) for n in ('hs', 'hs_tm', 'ru', 'rh', 'og')], hip._stream()))
        assert hip.lib.eve_last_kernel().decode() == name % ('fwd', fmt + '_t')
        hip._ck(hip.lib.eve_cgru_scan_bwd_c(dt_code(dt), B, T, C, p(d['dhs']), p(d['ru']), p(d['og']), p(d['hs_tm']), p(d['h0']), p(d['w1t']),
                                            p(d['w2t']), *[p(out_b[n][1]) for n in ('dg1', 'dg2', 'dxs', 'dh0')], hip._stream()))
        assert hip.lib.eve_last_kernel().decode() == name % ('bwd', fmt + '_t')
    torch.cuda.synchronize()
    check_guards(out_f, 'forward')
    check_guards(out_b, 'backward')
    for (n, (_, view)), want in list(zip(out_f.items(), want_f)) + list(zip(out_b.items(), want_b)):
        assert torch.equal(view, want), n
