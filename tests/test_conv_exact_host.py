"""CPU: the bit-exact convolution check (tests/exact_conv.py, tests/test_gpu_conv_exact.py) shown to bite without a GPU.

* the operand generators meet the two share conditions for the depth K and the format of every table row, by the reference alone;
* FakeKernels (CPU ATen) passes the exact check on a handful of small rows, every entry point;
* post-hoc corruptions of a correct result fail it, each in the regime meant to catch it.
"""
import pytest
import torch

import exact_conv as ec
import test_gpu_conv_exact as table
from fake_kernels import FakeKernels

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _depths():
    """(K, dtype, kind) of every 16-bit output the table checks.  kind: 'carried' (a bias or a previous tensor is added), 'plain_fwd' (the
    strided shortcut's forward, the stem: neither), 'plain_dgrad' (K = the fewest terms an output sums)."""
    seen = set()
    for r in table.CONV_ROWS:
        N, H, W, Cin, Cout, ks, stride, pad = r['shape']
        for dt in r['dtypes']:
            if dt == F32:
                continue
            for op in r['ops']:
                K = ks * ks * (Cin if op.startswith('fwd') else Cout)
                if op == 'dgrad':
                    seen.add((K // 9 if (stride == 2 and ks == 3) else K, dt, 'plain_dgrad'))
                else:
                    seen.add((K, dt, 'plain_fwd' if op == 'fwd_nobias' else 'carried'))
    for dt in ec.HALVES:
        seen.add((147, dt, 'plain_fwd'))         # the stem
    return sorted(seen, key=lambda t: (t[0], str(t[1]), t[2]))


@pytest.mark.parametrize('regime', ['exact', 'rounding'])
@pytest.mark.parametrize('K,dtype,kind', _depths(), ids=lambda v: ec.DT_ID.get(v, str(v)))
def test_generators_meet_their_share_conditions(K, dtype, kind, regime):
    """4 096 products of depth K from the value sets the rows use (+ bias where the entry point has one): the shares the GPU test
    asserts on its reference are reachable.  Only the plain data gradient below K = 576 is excused, and only from the tie share."""
    xv, wv, _ = (ec.value_sets if kind == 'carried' else ec.plain_value_sets)(regime, dtype, K)
    x, w = ec.pick((4096, K), xv, 1).double(), ec.pick((K,), wv, 2).double()
    s = x @ w
    if kind == 'carried':
        s = s + ec.gen_bias(4096, regime, dtype, K, 3).double()
    assert float(s.abs().max()) < ec.LIMIT
    assert all(float(torch.tensor(float(v)).to(dtype)) == v for v in xv), 'operands must be exact in the storage format'
    ec.check_regime(s, dtype, regime, 'K=%d %s' % (K, kind), ties_required=(kind != 'plain_dgrad' or K >= 576))


def _row(rows, name):
    return next(r for r in rows if r['id'] == name)


SMALL_CONV = ['1x1_s2_stream_64_128', 'halo_4_1_images', 'halo_2_2_images', 'dma_2_2', 'dma_s2_parity', 'igemm_f32_narrow', 'igemm_f32_wide',
              'igemm_prologue_narrow', 'wg8_2_4_4']
SMALL_WGRAD = ['wgrad_halo_1_1_3', 'wgrad_tr_1_4_0', 'wgrad_tr_2_2_1_s2', 'wgrad_v0_f32_narrow', 'wgrad_v0_16bit_narrow', 'wgrad_prologue_narrow',
               'wgrad_wg8_atomic']


@pytest.mark.parametrize('regime', ['exact', 'rounding'])
@pytest.mark.parametrize('name', SMALL_CONV)
def test_aten_restatement_passes_the_exact_check_forward_and_data_gradient(name, regime):
    r = _row(table.CONV_ROWS, name)
    for dt in r['dtypes']:
        ec.run_conv_row(ec.FakeCalls(FakeKernels()), r, dt, regime)


@pytest.mark.parametrize('regime', ['exact', 'rounding'])
@pytest.mark.parametrize('name', SMALL_WGRAD)
def test_aten_restatement_passes_the_exact_check_weight_gradient(name, regime):
    r = _row(table.WGRAD_ROWS, name)
    for dt in r['dtypes']:
        ec.run_wgrad_row(ec.FakeCalls(FakeKernels()), r, dt, regime)


def test_float32_reference_equals_float64_below_2_24():
    """The big rows take their reference in float32: the same integers."""
    x, w = ec.pick((2, 9, 12, 64), ec.signed([1, 2, 3, 4]), 1), ec.pick((128, 3, 3, 64), ec.signed([1, 2, 3]), 2)
    old = ec.REF64_MAX_MACS
    try:
        a = ec.ref_fwd(x, w, None, 1, 1)
        da = ec.ref_dgrad(a.float().clamp(-4, 4), w.permute(3, 1, 2, 0).contiguous(), (9, 12), 1, 1)
        wa = ec.ref_wgrad(x, a.float().clamp(-3, 3), 3, 3, 1, 1)[0]
        ec.REF64_MAX_MACS = 0.0
        b = ec.ref_fwd(x, w, None, 1, 1)
        db = ec.ref_dgrad(a.float().clamp(-4, 4), w.permute(3, 1, 2, 0).contiguous(), (9, 12), 1, 1)
        wb = ec.ref_wgrad(x, a.float().clamp(-3, 3), 3, 3, 1, 1)[0]
    finally:
        ec.REF64_MAX_MACS = old
    assert torch.equal(a, b) and torch.equal(da, db) and torch.equal(wa, wb)


# ---------------------------------------------------------------------------------------------- corruptions
def _case(regime, dtype, K=576, n=4096, with_prev=False):
    xv, wv, _ = ec.value_sets(regime, dtype, K)
    x, w = ec.pick((n, K), xv, 5).double(), ec.pick((K,), wv, 6).double()
    bias = ec.gen_bias(n, regime, dtype, K, 7).double()
    prev = ec.gen_prev((n,), regime, dtype, K, 8).double() if with_prev else torch.zeros(n, dtype=torch.float64)
    return x, w, bias, prev


def _fails(got, want):
    with pytest.raises(AssertionError, match='elements differ'):
        ec.check_exact(got, want, 'corrupted', ('m',))


@pytest.mark.parametrize('dtype', [BF, F16], ids=['bf16', 'f16'])
def test_one_lost_term_fails_in_the_exact_regime(dtype):
    x, w, bias, _ = _case('exact', dtype)
    want = x @ w + bias
    good = ec.round_once(want, dtype)
    ec.check_exact(good, ec.round_once(want, dtype), 'clean', ('m',))
    lost = want.clone()
    lost[1234] -= x[1234, 77] * w[77]                     # one channel at one pixel
    assert float(want[1234].abs()) <= ec.EXACT_CAP[dtype] - 2
    _fails(ec.round_once(lost, dtype), good)
    doubled = want.clone()
    doubled[7] += x[7, 0] * w[0]
    if float(want[7].abs()) <= ec.EXACT_CAP[dtype] - 2:
        _fails(ec.round_once(doubled, dtype), good)


def _truncate(v64, dtype):
    r = v64.float().to(dtype).double()
    u = ec.ulp_storage(v64, dtype)
    over = r.abs() > v64.abs()
    return torch.where(over, r - torch.sign(r) * ec.ulp_storage(r - torch.sign(r) * u / 2, dtype), r)


def _half_away(v64, dtype):
    r = v64.float().to(dtype).double()
    tie = ((r - v64).abs() * 2 == ec.ulp_storage(v64, dtype)) & (r != v64)
    away = v64 + torch.sign(v64) * (v64 - r).abs()
    return torch.where(tie, away, r)


@pytest.mark.parametrize('dtype', [BF, F16], ids=['bf16', 'f16'])
def test_wrong_roundings_fail_in_the_rounding_regime(dtype):
    x, w, bias, prev = _case('rounding', dtype, with_prev=True)
    s = x @ w
    want = s + bias + prev
    good = ec.round_once(want, dtype)
    # truncation toward zero instead of nearest even
    t = _truncate(want, dtype)
    assert torch.equal(t.float().to(dtype).double(), t) and bool((t.abs() <= want.abs()).all())
    _fails(t.float().to(dtype), good)
    # round half away from zero: differs from nearest even on half of the exact ties
    h = _half_away(want, dtype)
    assert torch.equal(h.float().to(dtype).double(), h)
    _fails(h.float().to(dtype), good)
    # the sum rounded to the storage format BEFORE bias / previous value are added
    twice = ec.round_once(ec.round_once(s, dtype).double() + bias + prev, dtype)
    _fails(twice, good)
    # partial sums passed through the storage format between two K chunks
    half = x.shape[1] // 2
    chunked = ec.round_once(ec.round_once(x[:, :half] @ w[:half] + bias + prev, dtype).double() + x[:, half:] @ w[half:], dtype)
    _fails(chunked, good)


def test_a_weight_gradient_off_by_one_in_a_two_million_pixel_sum_fails():
    """float32 dw: one entry off by 1 where the entries are sums over 2 M pixels (the bf16 tolerance of the older tests is ~1e4 there)."""
    M = 2 * 1024 * 1024
    x, dy = ec.pick((M, 8), ec.signed([1, 2]), 9), ec.pick((M, 4), ec.signed([1]), 10)
    ec.assert_below_2_24(2.0 * M + 900, 'dw')
    dw0 = ec.big_ints((4, 8), 300, 900, 11)
    want = dy.double().t() @ x.double() + dw0.double()
    got = (dy.t() @ x + dw0)                               # float32 accumulation of integers below 2^24: exact
    ec.check_exact(got, want, 'clean dw', ('o', 'i'))
    got[2, 5] += 1.0
    with pytest.raises(AssertionError, match=r'1 of 32 elements differ.*\n.*\(o, i\) = \(2, 5\)'):
        ec.check_exact(got, want, 'dw off by one', ('o', 'i'))


def test_guard_plane_and_non_finite_values_are_caught():
    buf, view = ec.guarded((2, 3, 3, 8), BF, 'cpu')
    view.zero_()
    ec.check_guard(buf, view, 'clean')
    buf[view.numel() + 5] = 0.0
    with pytest.raises(AssertionError, match='guard plane'):
        ec.check_guard(buf, view, 'written')
    bad = torch.zeros(4)
    bad[1] = float('inf')
    with pytest.raises(AssertionError, match='non-finite'):
        ec.check_exact(bad, torch.zeros(4), 'inf', ('m',))
    ec.check_exact(torch.tensor([-0.0]), torch.tensor([0.0]), 'signed zero', ('m',))
