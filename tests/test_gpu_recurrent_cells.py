"""GPU: EyeNet's recurrent scans (eve_amd/csrc/recurrent.hip, recurrent_wide.hip), their autograd shells (ops.GRUScanFn /
RNNScanFn / LSTMScanFn) and the conv-RNN gate kernels against float64 autograd of torch.nn.GRUCell / RNNCell / LSTMCell
(tests/recurrent_ref.py, pinned and shown to bite on planted defects by tests/test_recurrent_ref_host.py).

Every scan case is a CHAIN: the HIP forward, then the HIP backward on the tensors the HIP forward stored, everything compared with
float64 by close() of test_gpu_kernels.py (float32: 3e-5 x max|want|, 2e-5 relative L2); then the backward once more on the
float64-rounded forward tensors, so that a forward error cannot mask a backward one.

Which narrow kernel runs is decided by H alone (eve_gru_scan_fwd / _bwd: H == 128 is the register-resident GRU pair, every
other H <= 256 and every RNN / LSTM the generic one-thread-per-gate-row kernels); the narrow kernels do not take part in the
eve_last_kernel() attribution (test_gpu_wide_scans.py::test_narrow_scans_keep_their_kernels), the wide family is named here.

Recorded measurement (not asserted): the worst, over a family's cases and tensors, of
    (HIP error against float64) / (error of the float32 CPU restatement, tests/fake_kernels.py, against float64),
both as max|diff| / max|float64|, the restatement's error floored at 2^-24 (half a float32 spacing of the maximum):
    family                        gru    rnn   lstm
    narrow-generic               9.74   3.22   3.59
    narrow-h128                  2.52   1.54   3.79
    wide                         2.21   2.03   3.07
    narrow-generic saturated     3.21   1.49   1.74
    narrow-h128 saturated        0.88   3.13   1.61
    wide saturated               1.83   1.35   1.29
The largest figure is the generic GRU backward's dh0 (H = 256, T = 120: 2.2e-6 of max|dh0| against 2.3e-7 for the
restatement, a fourteenth of the bound): one thread sums the 3H products of a step in a single fmaf chain where ATen's matmul sums
in blocks; the H = 128 kernel splits the same sum in three.  Largest error of any tensor at any case: 3.3e-6 of its maximum
(hs of the wide RNN at H = 1024, T = 30, where the restatement has 2.3e-6), against the bound of 3e-5.
(narrow-h128 rnn / lstm run the generic cell kernels: only the GRU has a register-resident pair.)
"""
import pytest

import recurrent_ref as R
from fake_kernels import FakeKernels
from test_gpu_kernels import DTYPES, DT_IDS, dev, hip  # noqa: F401  (hip: the module-scoped fixture)

pytestmark = pytest.mark.gpu

BASELINE = FakeKernels()


def ident(v):
    return '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope='module')
def ratios():
    record = {}
    yield record
    for (fam, kind), r in sorted(record.items()):
        print('\nworst HIP error / restatement error: %-25s %-4s %.2f' % (fam, kind, r), end='')
    print()


class Named(object):
    """`hip`, remembering what eve_last_kernel() reads after each scan call."""

    def __init__(self, hip):
        self.hip, self.names = hip, []

    def __getattr__(self, name):
        fn = getattr(self.hip, name)
        if not (name.endswith('_scan_fwd') or name.endswith('_scan_bwd')):
            return fn

        def run(*a, **kw):
            out = fn(*a, **kw)
            self.names.append(self.hip.lib.eve_last_kernel().decode())
            return out
        return run


def check(hip, ratios, kind, H, S, T, with0, with_dcs, scale=1.0, plant=False):
    k = Named(hip)
    R.check_chain(k, R.reference(kind, H, S, T, with0, with_dcs, scale, plant), dev, baseline=BASELINE,
                  record=ratios, tag=' saturated' if plant else '')
    if H > 256:
        assert k.names == ['%s_scan_wide_%s_kernel' % (kind, d) for d in ('fwd', 'bwd', 'bwd')], k.names


# ------------------------------------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize('case', R.scan_grid(), ids=R.grid_id)
def test_scan_forward_then_backward_on_its_own_tensors(hip, ratios, case):
    """Widths 1, 3 (not a multiple of 4), 63 / 65 / 255 (either side of a wave), 128, 200, 256 (the LSTM's 1024 threads) at
    T = 1, 2 (the H = 128 prefetch's `t + 1 < T` / `t > 0` edges) and 30; T = 120; 300 sequences (more workgroups than CUs);
    the wide family at one full tile plus one row, T = 1, 2 (the double-buffered state's two halves), 30.  With and without
    an initial state; the LSTM also with dcs and no initial state, and the reverse."""
    kind, H, S, T, variants = case
    for with0, with_dcs in variants:
        check(hip, ratios, kind, H, S, T, with0, with_dcs)


# ------------------------------------------------------------------------------------------------ 2. saturated gates
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SAT_CASES, ids=ident)
def test_saturated_gates_stay_finite_and_exact(hip, ratios, kind, shape):
    """gi ~ 12 N(0, 1) with +-100 and +-1e4 planted in every gate block: e^x overflows float32 in both directions, a share of
    the gates sits at exactly 0 or +-1 (the host test holds the share between 20 % and 80 % on the float64 reference).
    Everything finite (close() asserts it) and equal to float64 under the same bound."""
    H, S, T = shape
    check(hip, ratios, kind, H, S, T, True, kind == 'lstm', R.SAT_SCALE, True)


# ------------------------------------------------------------------------------------------------ 3. the autograd shells
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SHELL_CASES, ids=ident)
def test_autograd_shells_against_the_nn_cells(hip, kind, shape):
    """ops.*ScanFn on CUDA leaf tensors: gradients of gi, w_hh, b_hh, h0, c0 -- _shift_states, _recurrent_param_grads and the
    needs_input_grad plumbing directly.  Variants: h0 = None; w_hh frozen with b_hh trained (`need_w or need_b`); the LSTM
    with only cs used downstream (dhs is None)."""
    H, S, T = shape
    for variant in R.shell_variants(kind):
        R.check_shell(*R.shell_reference(kind, H, S, T, variant), 'cuda', variant)


# ------------------------------------------------------------------------------------------------ 4. the gate kernels
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('which', range(4), ids=['one-vector', 'c24', 'beyond-the-grid-cap', 'saturated'])
def test_conv_rnn_gate_kernels(hip, dtype, which):
    """cgru_gates1 / 2, their backwards, clstm_gates_fwd / bwd (with and without dc_in) against float64: C = one vector, C = 24,
    one launch whose items exceed rgrid()'s 2048 x 256 so that the grid-stride loop takes a second turn, and planted +-100 /
    +-1e4 (float16: the largest finite value) gate inputs."""
    P, C, plant = R.gate_cases(dtype)[which]
    if which == 2:
        assert P * (C // R.VEC[dtype]) > 2048 * 256
    R.check_gates(hip, P, C, dtype, plant, dev)
