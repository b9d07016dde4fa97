"""CPU: pins tests/recurrent_ref.py -- the float64 references and comparison helpers that tests/test_gpu_recurrent_cells.py holds
the GRU / RNN / LSTM scans, their autograd shells and the conv-RNN gate kernels to.

  * the float64 restatement (the source of gates / hn_pre / dgh) equals the torch.nn cells under autograd to 1e-12;
  * FakeKernels (float32) passes the helpers at every case of the GPU grid; the printed error of that restatement against
    float64 is the figure the GPU error is reported against;
  * the same helpers FAIL on FakeKernels with one planted defect each -- the tests are shown to bite without a wrong kernel
    ever running on a GPU;
  * the saturated inputs saturate some gates and leave others live, and their gradients do not vanish.
"""
import pytest
import torch

import eve_amd
import recurrent_ref as R
from eve_amd import kernels, ops
from fake_kernels import FakeKernels

HERE = lambda t: t
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ['f32', 'bf16', 'fp16']


def ident(v):
    return '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('case', [(k, H, S, T) for k in R.KINDS for (H, S, T) in ((1, 1, 1), (3, 3, 2), (65, 3, 30), (128, 2, 120), (272, 17, 2))],
                         ids=ident)
def test_the_restatement_is_the_nn_cell_in_float64(case):
    kind, H, S, T = case
    for with0, with_dcs in R.variants(kind):
        c, want, rs = R.reference(kind, H, S, T, with0, with_dcs)
        for n in ('hs', 'cs', 'dgi', 'dwhh', 'dbhh', 'dh0', 'dc0'):
            assert (want[n] is None) == (rs[n] is None), n
            if want[n] is not None:
                err = float((want[n] - rs[n]).abs().max())
                assert err <= 1e-12 * max(1.0, float(want[n].abs().max())), (R.case_name(c), n, err)
        if kind == 'gru':                                   # dgh: dgi, its n-block times r
            r = rs['gates'][..., :H]
            assert float((rs['dgh'][..., :2 * H] - want['dgi'][..., :2 * H]).abs().max()) <= 1e-12
            assert float((rs['dgh'][..., 2 * H:] - want['dgi'][..., 2 * H:] * r).abs().max()) <= 1e-12


def test_the_saturated_reference_matches_the_nn_cell_too():
    for kind in R.KINDS:
        c, want, rs = R.reference(kind, 65, 3, 8, True, kind == 'lstm', R.SAT_SCALE, True)
        for n in ('hs', 'cs', 'dgi', 'dh0', 'dc0'):
            if want[n] is not None:
                assert float((want[n] - rs[n]).abs().max()) <= 1e-12 * max(1.0, float(want[n].abs().max())), (kind, n)


# ------------------------------------------------------------------------------------------------ FakeKernels passes
@pytest.mark.parametrize('case', R.scan_grid(), ids=R.grid_id)
def test_the_float32_restatement_passes_every_case_of_the_gpu_grid(case):
    kind, H, S, T, variants = case
    for with0, with_dcs in variants:
        R.check_chain(FakeKernels(), R.reference(kind, H, S, T, with0, with_dcs), HERE)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SAT_CASES, ids=ident)
def test_the_float32_restatement_passes_the_saturated_cases(kind, shape):
    H, S, T = shape
    R.check_chain(FakeKernels(), R.reference(kind, H, S, T, True, kind == 'lstm', R.SAT_SCALE, True), HERE)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SAT_CASES, ids=ident)
def test_the_saturated_inputs_saturate_some_gates_and_keep_gradients_alive(kind, shape):
    """On the float64 reference alone.  The saved activations (GRU r, z, n; LSTM i, f, g, o; the RNN's tanh output) within 1e-6
    of 0 or +-1 make up between 20 % and 80 %: saturated and live elements are both present; dgi and dh0 do not vanish."""
    H, S, T = shape
    c, want, rs = R.reference(kind, H, S, T, True, kind == 'lstm', R.SAT_SCALE, True)
    g = rs['gates'] if kind != 'rnn' else rs['hs']
    share = float(((g.abs() < 1e-6) | ((g.abs() - 1).abs() < 1e-6)).double().mean())
    print('%s H%d: saturated share %.3f, |h| > 0.999 share %.3f, max|dgi| %.3e, max|dh0| %.3e' % (
        kind, H, share, float((want['hs'].abs() > 0.999).double().mean()), float(want['dgi'].abs().max()), float(want['dh0'].abs().max())))
    assert 0.2 <= share <= 0.8
    assert float(want['dgi'].abs().max()) > 1e-3
    assert float(want['dh0'].abs().max()) > 1e-3
    assert float(c['gi'].max()) == 1e4 and float(c['gi'].min()) == -1e4
    for b in range(R.G_OF[kind]):
        block = c['gi'][..., b * H:(b + 1) * H]
        assert {100.0, -100.0, 1e4, -1e4} <= set(block[block.abs() >= 100].tolist())


# ------------------------------------------------------------------------------------------------ the shells
@pytest.fixture()
def fake():
    k = FakeKernels()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SHELL_CASES, ids=ident)
def test_the_autograd_shells_pass_under_the_float32_restatement(fake, kind, shape):
    H, S, T = shape
    for variant in R.shell_variants(kind):
        R.check_shell(*R.shell_reference(kind, H, S, T, variant), 'cpu', variant)


# ------------------------------------------------------------------------------------------------ the gate kernels
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_the_gate_restatement_passes_every_case_of_the_gpu_grid(dtype):
    for P, C, plant in R.gate_cases(dtype):
        R.check_gates(FakeKernels(), P, C, dtype, plant, HERE)


def test_the_gate_backward_references_read_only_what_the_kernels_are_given():
    """gates2's adjoint has no reset-gate term; gates1's adjoint does not read dru's reset half."""
    o = R.gate_operands(9, 8, torch.float32, False)
    ru, _ = R.cgru_gates1_f64(o['g1'], o['h'])
    og, _ = R.cgru_gates2_f64(o['g2'], ru, o['h'])
    dg2, dru, dh = R.cgru_gates2_bwd_f64(o['dhnew'], ru, o['h'], og)
    assert float(dru[..., :8].abs().max()) == 0.0 and float(dru[..., 8:].abs().max()) > 0
    other = o['dru'].clone()
    other[..., :8] = 7.0
    for a, b in zip(R.cgru_gates1_bwd_f64(o['drh'], o['dru'], ru, o['h']), R.cgru_gates1_bwd_f64(o['drh'], other, ru, o['h'])):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ sensitivity
class NoH0InGruBackward(FakeKernels):
    """h0 ignored at t = 0 in the GRU backward's h_{t-1}."""
    def gru_scan_bwd(self, dhs, whh, h0, hs, gates, hn_pre, want_dh0):
        return super().gru_scan_bwd(dhs, whh, None, hs, gates, hn_pre, want_dh0)


class DghWithoutR(FakeKernels):
    """dgh's n-block not multiplied by r."""
    def gru_scan_bwd(self, dhs, whh, h0, hs, gates, hn_pre, want_dh0):
        dgi, dgh, dh0 = super().gru_scan_bwd(dhs, whh, h0, hs, gates, hn_pre, want_dh0)
        H = dhs.shape[2]
        dgh[..., 2 * H:] = dgi[..., 2 * H:]
        return dgi, dgh, dh0


class NoC0InLstmBackward(FakeKernels):
    """LSTM c_{t-1} at t = 0 taken as 0 despite c0."""
    def lstm_scan_bwd(self, dhs, dcs, whh, c0, hs, cs, gates, want_d0):
        return super().lstm_scan_bwd(dhs, dcs, whh, None, hs, cs, gates, want_d0)


class DcCarryWithoutF(FakeKernels):
    """The carried dc not multiplied by the forget gate."""
    def lstm_scan_bwd(self, dhs, dcs, whh, c0, hs, cs, gates, want_d0):
        S, T, H = dhs.shape
        dh, dc = torch.zeros((S, H)), torch.zeros((S, H))
        dpre = torch.zeros((S, T, 4 * H))
        for t in range(T - 1, -1, -1):
            dd = dh + dhs[:, t]
            i, f, g, o = gates[:, t].chunk(4, dim=1)
            tc = torch.tanh(cs[:, t])
            cp = cs[:, t - 1] if t > 0 else (c0 if c0 is not None else torch.zeros((S, H)))
            dc = dc + (dcs[:, t] if dcs is not None else 0) + dd * o * (1 - tc * tc)
            dpre[:, t] = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dd * tc * o * (1 - o)], 1)
            dh = dpre[:, t] @ whh                           # ... and dc goes on as it is
        return dpre, (dh if want_d0 else None), (dc * gates[:, 0, H:2 * H] if want_d0 else None)


class GateOrderIFOG(FakeKernels):
    """The LSTM's blocks read as i, f, o, g instead of i, f, g, o."""
    def lstm_scan_fwd(self, gi, whh_t, bhh, h0, c0):
        H = gi.shape[2] // 4
        perm = torch.cat([torch.arange(0, 2 * H), torch.arange(3 * H, 4 * H), torch.arange(2 * H, 3 * H)])
        return super().lstm_scan_fwd(gi[..., perm], whh_t[:, perm], bhh[perm], h0, c0)


class LastUnitZero(FakeKernels):
    """The last hidden unit (j = H - 1) left at zero."""
    def gru_scan_fwd(self, gi, whh_t, bhh, h0):
        hs, gates, hn_pre = super().gru_scan_fwd(gi, whh_t, bhh, h0)
        hs[..., -1] = 0
        return hs, gates, hn_pre


class LastSequenceNotWritten(FakeKernels):
    """The last sequence (s = S - 1) not written."""
    def rnn_scan_bwd(self, dhs, whh, hs, want_dh0):
        dpre, dh0 = super().rnn_scan_bwd(dhs, whh, hs, want_dh0)
        dpre[-1] = 0
        return dpre, dh0


KERNEL_DEFECTS = [(NoH0InGruBackward, 'gru', True, False), (DghWithoutR, 'gru', False, False), (NoC0InLstmBackward, 'lstm', True, True),
                  (DcCarryWithoutF, 'lstm', False, True), (GateOrderIFOG, 'lstm', False, False), (LastUnitZero, 'gru', False, False),
                  (LastSequenceNotWritten, 'rnn', False, False)]


@pytest.mark.parametrize('defect', KERNEL_DEFECTS, ids=lambda v: v[0].__name__)
@pytest.mark.parametrize('shape', [(65, 3, 2), (128, 3, 30), (272, 17, 2)], ids=ident)
def test_a_planted_kernel_defect_fails_the_chain_comparison(defect, shape):
    cls, kind, with0, with_dcs = defect
    H, S, T = shape
    case = R.reference(kind, H, S, T, with0, with_dcs)
    R.check_chain(FakeKernels(), case, HERE)                # the same case passes without the defect
    with pytest.raises(AssertionError):
        R.check_chain(cls(), case, HERE)
    print('%s (%s) fails at %s' % (cls.__name__, cls.__doc__, R.case_name(case[0])))


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SHELL_CASES[:2] + R.SHELL_CASES[-1:], ids=ident)
def test_a_state_shift_off_by_one_fails_the_shell_comparison(fake, monkeypatch, kind, shape):
    H, S, T = shape
    c, want = R.shell_reference(kind, H, S, T, 'all')
    R.check_shell(c, want, 'cpu', 'all')

    def shifted_one_step_too_far(first, hs):                # rows h_{t-2} instead of h_{t-1}
        S_, T_, H_ = hs.shape
        z = torch.zeros((S_, 1, H_))
        return torch.cat([z, (first if first is not None else z[:, 0]).unsqueeze(1), hs[:, :-2]], dim=1).reshape(S_ * T_, H_).contiguous()
    monkeypatch.setattr(ops, '_shift_states', shifted_one_step_too_far)
    with pytest.raises(AssertionError, match='dW_hh'):
        R.check_shell(c, want, 'cpu', 'all')
