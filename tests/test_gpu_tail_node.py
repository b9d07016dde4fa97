"""GPU: the EyeNet train step's tail node (ops.EyeTailLossFn) and the kernels only it launches, against float64 (tests/tail_ref.py;
tests/test_tail_ref_host.py pins the references and shows that the bounds bite).

  (a) linear_wgrad_batch_kernel on random operands inside the bound of ANY correct float32 algorithm (derived in tail_ref, not
      measured): the shifted X of the recurrent weight across split boundaries, the nine problems of the product step in one
      launch (the first_block table, the `more` prefetch branch), [X | X2], K1 < K, wide dY / Y, masked sizes, a full batch of
      twelve, and the refusals;
  (b) the same kernel on integer-valued operands, where float atomics in any order give the exact integer: `==`;
  (c) tail_head_pose / tail_outputs_fwd / tail_outputs_bwd directly, in one block, with two rows in a second block, and across
      the left / right switch;
  (d) sum_rows_pairs;
  (e) the node itself against float64 autograd of the same chain.

Every output is caller-owned with a guard region behind it and every launch is made twice; eve_last_kernel() names the kernel.
Each case asserts, through tail_ref.expected_splits or the kernel name, that it reaches the situation it is named for.

Measured on an MI355X (every test prints its figures): (a) max err / bound 0.007 on the product batches, 0.009 on the shift,
X2, K1 < K and wide-dY cases, 0.063 on the masked sizes, 0.137 on the 1 x 1 x 1 problem of the full batch -- the float32
restatement's own figures; (c) gaze within 0.94 float32 spacings, d_g2 within 1.59, d_p2 within 0.94; (d) at most 0.36 of
the bound; (e) in the node test's docstring.  The whole module runs in under 4 s.
"""
import pytest
import torch

import exact_conv as ec
import tail_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
WGRAD = 'linear_wgrad_batch_kernel'


@pytest.fixture(scope='module')
def hip():
    from eve_amd.kernels import HipKernels
    assert torch.cuda.is_available(), 'GPU suite needs a GPU'
    return HipKernels()


def last(hip):
    return hip.lib.eve_last_kernel().decode()


# ------------------------------------------------------------------------------------------------ (a), (b): the batched weight gradient
def on_device(p):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in p.items() if k not in ('dW', 'db')}


def run_wgrad(hip, problems, what):
    """One linear_wgrad_batch call on `problems`, twice, each time from the problems' dW / db values: all outputs live in ONE
    buffer (dW0, db0, dW1, ...) with the guard region behind it.  -> per launch [(dW, db or None)] on the CPU."""
    parts = []
    for p in problems:
        parts.append(p['dW'].reshape(-1))
        if p.get('db') is not None:
            parts.append(p['db'])
    base = torch.cat(parts)
    dev = [on_device(p) for p in problems]

    def split(out):
        res, o = [], 0
        for p in problems:
            n = p['dW'].numel()
            dw = out[o:o + n].view(*p['dW'].shape)
            o += n
            db = None
            if p.get('db') is not None:
                db = out[o:o + p['db'].numel()]
                o += p['db'].numel()
            res.append((dw, db))
        assert o == out.numel()
        return res

    launches = []
    for _ in range(2):
        buf, view = ec.guarded((base.numel(),), F32, 'cuda')
        view.copy_(base.cuda())
        hip.linear_wgrad_batch([dict(d, dW=dw, db=db) for d, (dw, db) in zip(dev, split(view))])
        assert last(hip) == WGRAD, '%s ran on %s' % (what, last(hip))
        ec.check_guard(buf, view, what)
        launches.append([(dw.cpu(), None if db is None else db.cpu()) for dw, db in split(view)])
    return launches


def check_bound(hip, problems, what):
    """Both launches of an atomics kernel meet the bound (they need not be bit-equal)."""
    refs = [R.wgrad_batch_f64(p) for p in problems]
    for n, launch in enumerate(run_wgrad(hip, problems, what)):
        for i, ((dw, db), ref, p) in enumerate(zip(launch, refs, problems)):
            rw, rb = R.bound_ratios(dw, db, ref)
            print('%-34s launch %d #%-2d %-12s dW err/bound %.4f  db %s' % (what, n, i, 'x'.join(map(str, R.problem_dims(p)[:3])), rw,
                                                                          '-' if rb is None else '%.4f' % rb))
            assert rw <= 1.0, '%s #%d: a dW entry is %.3f x its bound away from float64' % (what, i, rw)
            assert rb is None or rb <= 1.0, '%s #%d: a db entry is %.3f x its bound away from float64' % (what, i, rb)
            K1, K2 = R.problem_dims(p)[3:]
            assert torch.equal(dw[:, K1 + K2:], p['dW'][:, K1 + K2:]), '%s #%d: columns of dW beyond K1 + K2 changed' % (what, i)


def assert_shift_case_reaches_its_splits(problems):
    """>= 3 splits, a split boundary that is no multiple of T (inside a sequence), a ragged last split."""
    s, T = R.expected_splits(problems)[0], problems[0]['x_shift_T']
    assert len(s['sizes']) >= 3 and s['rows'] % T != 0 and s['sizes'][-1] % 64 != 0 and s['sizes'][-1] < s['rows'], s


def assert_product_case_reaches_its_splits(problems, T, prefetch):
    sp = R.expected_splits(problems)
    assert len(problems) > 1 and all(e['first_block'] > 0 for e in sp[1:])                   # the first_block table is walked
    shifted = [e for e, p in zip(sp, problems) if p.get('x_shift_T')]
    assert shifted and all(len(e['sizes']) >= 2 and e['rows'] % T != 0 for e in shifted)       # a split boundary inside a sequence
    if prefetch:                                         # more than 8 sixteen-row blocks in a split: the `more` prefetch branch runs
        assert all(max(e['sizes']) > 128 for e in sp)


BOUND = R.bound_cases()


def test_wgrad_batch_shifted_x_across_split_boundaries(hip):
    ps = BOUND['shift M130 T13']
    assert_shift_case_reaches_its_splits(ps)
    check_bound(hip, ps, 'shift M130 T13')


@pytest.mark.parametrize('name,T,prefetch', [('product B4 T30', 30, False), ('product B8 T30', 30, True), ('product B4 T30, parameter shapes', 30, False)])
def test_wgrad_batch_the_nine_product_problems_in_one_call(hip, name, T, prefetch):
    ps = BOUND[name]
    assert len(ps) == 9 and sum(e['tiles'] for e in R.expected_splits(ps)) == 236
    assert_product_case_reaches_its_splits(ps, T, prefetch)
    check_bound(hip, ps, name)


def test_wgrad_batch_concatenated_x_and_short_k1(hip):
    """[X | X2] gives the gradient on the concatenation; with K1 < K and no X2 the trailing columns keep their base value exactly
    (check_bound compares them with torch.equal)."""
    p = BOUND['X2 128+2'][0]
    cat = dict(p, X=torch.cat([p['X'], p['X2']], dim=1), K1=130)
    del cat['X2']
    a, b = R.wgrad_batch_f64(p), R.wgrad_batch_f64(cat)
    assert torch.equal(a['dW'], b['dW']) and float((a['dW'][:, 128:] - p['dW'][:, 128:].double()).abs().min()) > 0
    check_bound(hip, [p], 'X2 128+2')
    q = BOUND['K1 < K'][0]
    assert R.problem_dims(q)[3:] == (128, 0) and q['dW'].shape[1] == 130
    check_bound(hip, [q], 'K1 < K')


def test_wgrad_batch_wide_dy(hip):
    p = BOUND['wide dY SELU'][0]
    assert p['dY'].shape[1] == R.problem_dims(p)[1] + 4 and p['Y'].shape == p['dY'].shape and p['act'] == R.ACT_SELU
    check_bound(hip, [p], 'wide dY SELU')


@pytest.mark.parametrize('mnk', R.MASKED_MNK, ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_batch_masked_sizes(hip, mnk):
    name = 'masked %dx%dx%d' % mnk
    check_bound(hip, BOUND[name], name)


def test_wgrad_batch_full_batch(hip):
    ps = BOUND['full batch']
    assert len(ps) == R.WGRAD_BATCH_MAX and {p['act'] for p in ps} == set(range(6))
    check_bound(hip, ps, 'full batch')


def problem_array(problems, n=None):
    """The eve_wgrad_problem array of HipKernels.linear_wgrad_batch, for calls its assertions would stop."""
    from eve_amd import _lib
    arr = (_lib.WgradProblem * (n or len(problems)))()
    for q, p in zip(arr, problems):
        ptr = lambda t: None if t is None else t.data_ptr()
        q.dY, q.Y, q.X, q.X2, q.dW, q.db = ptr(p['dY']), ptr(p.get('Y')), ptr(p['X']), ptr(p.get('X2')), ptr(p['dW']), ptr(p.get('db'))
        q.M, q.N, q.K = p['dY'].shape[0], p['dY'].shape[1], p['X'].shape[1]
        q.K1, q.K2, q.act = q.K, 0, p.get('act', 0)
    return arr


def test_wgrad_batch_refusals(hip):
    """n = 0, n > WGRAD_BATCH_MAX, K1 > K, an activation without Y and a NULL dW return an error: nothing is launched (the last
    kernel's name stays) and the outputs keep their values."""
    p = R.make_problem(40, 8, 16, 5)
    buf, view = ec.guarded((8 * 16 + 8,), F32, 'cuda')
    base = torch.cat([p['dW'].reshape(-1), p['db']]).cuda()
    view.copy_(base)
    d = dict(on_device(p), dW=view[:128].view(8, 16), db=view[128:])
    g2 = torch.zeros((4, 4), device='cuda')
    hip.tail_outputs_fwd(g2, g2)
    assert last(hip) == 'tail_outputs_fwd_kernel'

    def refused(arr, n):
        status = hip.lib.eve_linear_wgrad_batch(arr, n, hip._stream())
        assert status != 0
        with pytest.raises(RuntimeError, match='linear_wgrad_batch'):
            hip._ck(status)
        torch.cuda.synchronize()
        assert last(hip) == 'tail_outputs_fwd_kernel' and torch.equal(view, base)
        ec.check_guard(buf, view, 'refusal')

    refused(problem_array([d]), 0)
    refused(problem_array([d] * (R.WGRAD_BATCH_MAX + 1)), R.WGRAD_BATCH_MAX + 1)
    arr = problem_array([d]); arr[0].K1 = arr[0].K + 1
    refused(arr, 1)
    arr = problem_array([d]); arr[0].act = R.ACT_SELU
    refused(arr, 1)
    arr = problem_array([d]); arr[0].dW = None
    refused(arr, 1)
    arr = problem_array([d, d]); arr[1].dW = None                   # the bad problem behind a good one: still nothing runs
    refused(arr, 2)
    hip._ck(hip.lib.eve_linear_wgrad_batch(problem_array([d]), 1, hip._stream()))        # ... and the array itself is a valid call
    assert last(hip) == WGRAD and not torch.equal(view, base)


EXACT = R.exact_cases()


@pytest.mark.parametrize('name', sorted(EXACT))
def test_wgrad_batch_exact_on_integer_operands(hip, name):
    ps = EXACT[name]
    sp = R.expected_splits(ps)
    if name.startswith('shift'):
        assert_shift_case_reaches_its_splits(ps)
    elif name.startswith('product'):
        assert {p['act'] for p in ps} == {R.ACT_NONE, R.ACT_RELU}
        assert_product_case_reaches_its_splits(ps, 30, False)
    else:
        assert len(sp[0]['sizes']) == 31 and sp[0]['sizes'][-1] == 1
    refs = [R.wgrad_batch_f64(p) for p in ps]
    a, b = run_wgrad(hip, ps, name)
    for i, ref in enumerate(refs):
        for launch in (a, b):
            ec.check_exact(launch[i][0], ref['dW'], '%s #%d dW' % (name, i), ('n', 'k'))
            if ref['db'] is not None:
                ec.check_exact(launch[i][1], ref['db'], '%s #%d db' % (name, i), ('n',))


# ------------------------------------------------------------------------------------------------ (c): the small tail kernels
SMALL_BT = (1, 128, 129, 150)        # 2 BT = 256 fills one block, 258 puts two rows into a second, 300 crosses the switch there


def ulps(got, want64):
    """|got - want| in float32 spacings at want"""
    return float(((got.detach().cpu().double() - want64).abs() / R.ulp32(want64).clamp_min(2.0 ** -149)).max())


@pytest.mark.parametrize('ld,col', [(132, 128), (136, 128)])
@pytest.mark.parametrize('BT', SMALL_BT)
def test_tail_head_pose_fills_its_four_columns_only(hip, BT, ld, col):
    hl, hr = R.rnd((BT, 2), 3 * BT), R.rnd((BT, 2), 3 * BT + 1)
    hld, hrd = hl.cuda(), hr.cuda()
    got = ec.launch_twice(ec.HipCalls(hip), 'tail_head_pose', 'tail_head_pose_kernel', F32, (2 * BT, ld), F32, None,
                          lambda out: hip.tail_head_pose(hld, hrd, out, col))
    want = R.head_pose_f64(torch.full((2 * BT, ld), ec.GUARD_VALUE), hl, hr, col)
    ec.check_exact(got, want, 'tail_head_pose BT %d ld %d' % (BT, ld), ('m', 'c'))
    assert (2 * BT + 255) // 256 == (1 if BT <= 128 else 2)


def test_tail_head_pose_refuses_a_bad_stride_or_column(hip):
    h = torch.zeros((4, 2), device='cuda')
    buf, cat = ec.guarded((8, 136), F32, 'cuda')
    hip.tail_outputs_fwd(torch.zeros((4, 4), device='cuda'), torch.zeros((4, 4), device='cuda'))
    for ld, col in ((134, 128), (136, 130), (128, 128), (136, 136)):
        status = hip.lib.eve_tail_head_pose(4, hip._p(h), hip._p(h), hip._p(cat), ld, col, hip._stream())
        assert status != 0, (ld, col)
        with pytest.raises(RuntimeError, match='tail_head_pose'):
            hip._ck(status)
    torch.cuda.synchronize()
    assert last(hip) == 'tail_outputs_fwd_kernel' and bool((buf == ec.GUARD_VALUE).all())


@pytest.mark.parametrize('BT', SMALL_BT)
def test_tail_outputs_fwd(hip, BT):
    M = 2 * BT
    g2, p2 = torch.tanh(R.rnd((M, 4), 5 * BT)), R.rnd((M, 4), 5 * BT + 1).clamp(min=0)
    g2d, p2d = g2.cuda(), p2.cuda()

    def fn(out):                                         # gaze [M, 2] and pupil [M] in one buffer: the guard sits behind pupil
        hip._ck(hip.lib.eve_tail_outputs_fwd(M, hip._p(g2d), hip._p(p2d), hip._p(out[:2 * M]), hip._p(out[2 * M:]), hip._stream()))
    got = ec.launch_twice(ec.HipCalls(hip), 'tail_outputs_fwd', 'tail_outputs_fwd_kernel', F32, (3 * M,), F32, None, fn).cpu()
    gaze, pupil = R.outputs_fwd_f64(g2, p2)
    u = ulps(got[:2 * M].view(M, 2), gaze)
    print('tail_outputs_fwd BT %d: gaze within %.2f float32 spacings of float64' % (BT, u))
    assert u <= 1.0
    ec.check_exact(got[2 * M:], pupil, 'tail_outputs_fwd pupil', ('m',))


@pytest.mark.parametrize('with_upstream', [False, True], ids=['g_full_none', 'g_full_device'])
@pytest.mark.parametrize('BT', SMALL_BT)
def test_tail_outputs_bwd(hip, BT, with_upstream):
    M = 2 * BT
    dg, dp = [R.rnd((BT, 2), 7 * BT + i) for i in range(2)], [R.rnd((BT,), 7 * BT + 2 + i) for i in range(2)]
    up = torch.tensor([0.37], dtype=F32) if with_upstream else None
    c_ang, c_l1 = 1.25, 0.3
    dgd, dpd, upd = [t.cuda() for t in dg], [t.cuda() for t in dp], (up.cuda() if with_upstream else None)

    def fn(out):                                         # d_g2, then d_p2, [M, 4] each
        hip._ck(hip.lib.eve_tail_outputs_bwd(BT, hip._p(dgd[0]), hip._p(dgd[1]), hip._p(dpd[0]), hip._p(dpd[1]), hip._p(upd), c_ang, c_l1,
                                             hip._p(out[:M]), hip._p(out[M:]), hip._stream()))
    got = ec.launch_twice(ec.HipCalls(hip), 'tail_outputs_bwd', 'tail_outputs_bwd_kernel', F32, (2 * M, 4), F32, None, fn).cpu()
    # (the kernel takes the coefficients as float32)
    c32 = lambda c: float(torch.tensor(c, dtype=F32))
    d_g2, d_p2 = R.outputs_bwd_f64(dg[0], dg[1], dp[0], dp[1], up, c32(c_ang), c32(c_l1))
    ug, up_ = ulps(got[:M, :2], d_g2[:, :2]), ulps(got[M:, :1], d_p2[:, :1])
    print('tail_outputs_bwd BT %d: d_g2 within %.2f, d_p2 within %.2f float32 spacings of float64' % (BT, ug, up_))
    assert ug <= 3.0 and up_ <= 3.0
    assert bool((got[:M, 2:] == 0).all()) and bool((got[M:, 1:] == 0).all()), 'the padded columns are exactly 0'


# ------------------------------------------------------------------------------------------------ (d): sum_rows_pairs
@pytest.mark.parametrize('rows,C', [(1, 8), (15, 16), (17, 33), (960, 32)])
def test_sum_rows_pairs_adds_in_place_in_a_fixed_order(hip, rows, C):
    sums, o0, o1 = R.rnd((rows, C, 2), rows + C), R.rnd((C,), rows + C + 1, 3.0), R.rnd((C,), rows + C + 2, 3.0)
    sd = sums.cuda()
    outs = []
    for _ in range(2):
        pair = []
        for o in (o0, o1):                               # each vector is followed by its own guard: elements beyond C stay
            buf, view = ec.guarded((C,), F32, 'cuda')
            view.copy_(o.cuda())
            pair.append((buf, view))
        hip.sum_rows_pairs(sd, pair[0][1], pair[1][1])
        for buf, view in pair:
            ec.check_guard(buf, view, 'sum_rows_pairs')
        outs.append([view.cpu() for _, view in pair])
    ref = R.sum_rows_pairs_f64(sums, o0, o1)
    for j in range(2):
        assert torch.equal(outs[0][j], outs[1][j]), 'sum_rows_pairs: the same launch twice gives different results'
        want, bound = ref[j]
        r = float(((outs[0][j].double() - want).abs() / bound).max())
        print('sum_rows_pairs %dx%d out%d err/bound %.3f' % (rows, C, j, r))
        assert r <= 1.0


# ------------------------------------------------------------------------------------------------ (e): the node
@pytest.fixture(scope='module')
def node_net():
    """The net and train.eyenet_trainer as tests/test_gpu_eyenet.py builds them (the flat gradients exist), the last gaze layer
    with a signal."""
    import eve_amd
    from eve_amd import train
    from oracle import detweights
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict({'batch_size': 16, 'weight_decay': 0.005, 'base_learning_rate': 0.001})
    net = eve_amd.EyeNet()
    net.compute_dtype = F32
    detweights.fill_module(net, seed=0)
    net = net.cuda()
    with torch.no_grad():
        g = torch.Generator().manual_seed(12)
        net.fc_to_gaze[2].weight.copy_(0.05 * torch.randn(net.fc_to_gaze[2].weight.shape, generator=g).cuda())
    tr = train.eyenet_trainer(net, net.config)
    return net, tr


NODE_CASES = [(B, T, False) for B, T in R.NODE_BT] + [(3, 5, True)]


@pytest.mark.parametrize('B,T,right_invalid', NODE_CASES, ids=['B%d-T%d%s' % (B, T, '-right-eye-invalid' if r else '') for B, T, r in NODE_CASES])
def test_tail_node_against_float64_autograd(hip, node_net, B, T, right_invalid):
    """ops.EyeTailLossFn.apply on a random float32 leaf `feats` [2 B T, 512] (no trunk runs): the five terms, gaze, pupil, hs,
    d(feats) and the 17 parameter gradients (p.grad itself, the flat gradient zeroed before) against tail_ref.tail_f64 on the same
    weights and inputs.  Per tensor the tolerance is max(4 x the deviation of the float32 CPU chain (tail_ref.tail_f32) from
    float64, 1e-6 max(1, max |want|)).

    Measured on an MI355X: the case with the largest error / tolerance per tensor, over the six cases (max 0.56; no case misses).
    tensor                     err/tol  GPU err  f32 chain  tolerance  case
    term ang_l                 0.11   5.9e-06  2.1e-06  5.6e-05  B8 T30
    term l1_l                  0.05   9.5e-08  1.4e-07  1.8e-06  B2 T33
    term ang_r                 0.19   6.2e-06  5.3e-06  3.2e-05  B1 T1
    term l1_r                  0.17   4.8e-07  7.2e-07  2.9e-06  B1 T1
    term full                  0.15   1.7e-05  2.2e-06  1.2e-04  B8 T30
    gaze                       0.27   1.2e-06  1.1e-06  4.3e-06  B3 T5
    pupil                      0.20   1.3e-06  1.6e-06  6.4e-06  B3 T5
    hs                         0.29   4.2e-06  3.6e-06  1.4e-05  B2 T33
    d_feats                    0.27   4.3e-06  4.1e-06  1.6e-05  B3 T5
    d cnn_layers.fc.weight     0.29   2.3e-05  2.0e-05  8.2e-05  B1 T1
    d cnn_layers.fc.bias       0.35   1.6e-05  1.1e-05  4.5e-05  B1 T1
    d fc_common.0.weight       0.33   3.1e-05  2.4e-05  9.5e-05  B1 T1
    d fc_common.0.bias         0.34   1.3e-05  9.3e-06  3.7e-05  B1 T1
    d fc_common.2.weight       0.24   1.7e-05  1.8e-05  7.1e-05  B3 T5
    d fc_common.2.bias         0.27   6.3e-06  5.8e-06  2.3e-05  B1 T1
    d rnn_cells.0.weight_ih    0.49   5.9e-05  3.0e-05  1.2e-04  B1 T1
    d rnn_cells.0.bias_ih      0.56   1.2e-05  5.2e-06  2.1e-05  B1 T1
    d rnn_cells.0.weight_hh    0.24   1.9e-06  2.0e-06  7.9e-06  B2 T33
    d rnn_cells.0.bias_hh      0.43   8.4e-06  5.0e-06  2.0e-05  B1 T1
    d fc_to_gaze.0.weight      0.28   2.5e-05  2.2e-05  8.8e-05  B1 T1
    d fc_to_gaze.0.bias        0.41   7.6e-06  4.6e-06  1.8e-05  B3 T5
    d fc_to_gaze.2.weight      0.54   5.8e-05  2.7e-05  1.1e-04  B3 T5, right eye invalid
    d fc_to_pupil.0.weight     0.32   7.1e-07  5.7e-07  2.3e-06  B1 T1
    d fc_to_pupil.0.bias       0.34   3.4e-07  2.0e-07  1.0e-06  B1 T1
    d fc_to_pupil.2.weight     0.26   1.7e-06  1.6e-06  6.4e-06  B1 T1
    d fc_to_pupil.2.bias       0.03   3.2e-08  2.8e-08  1.0e-06  B5 T30
    Every case takes under 0.1 s (the first one 0.7 s: it builds the net and the trainer).
    """
    from eve_amd import ops
    net, tr = node_net
    c_ang, c_l1 = float(net.config.loss_coeff_g_ang_initial), float(net.config.loss_coeff_pupil_size)
    feats, hl, hr, tgt = R.node_case(B, T, right_invalid)
    params = ops.EyeTailLossFn.tail_parameters(net)
    assert len(params) == 17 and all(ops._direct_grad_ok(p) for p in params)
    names = {id(p): n for n, p in net.named_parameters()}
    assert [names[id(p)] for p in params] == list(R.TAIL_KEYS)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k in R.TAIL_KEYS}
    tr.fp.zero_grad()
    P = net._get_packs()
    packs = tuple(P[n] for n in ('fc', 'fc_common.0', 'fc_common.2', 'rnn.0.ih', 'rnn.0.hh', 'fc_to_gaze.0', 'fc_to_gaze.2',
                                 'fc_to_pupil.0', 'fc_to_pupil.2'))
    x = feats.cuda().requires_grad_(True)
    out = ops.EyeTailLossFn.apply(x, hl.cuda(), hr.cuda(), tuple(t.cuda() for t in tgt), c_ang, c_l1, net, packs, B, T)
    # the node, not the per-layer path: ONE autograd node made every output (its backward runs on autograd's own thread, and
    # eve_last_kernel() is per thread: the kernel names are held by the direct tests above)
    assert type(out[4].grad_fn).__name__ == 'EyeTailLossFnBackward' and all(o.grad_fn is out[4].grad_fn for o in out[:5])
    out[4].backward()
    torch.cuda.synchronize()
    got = {'terms': torch.stack([o.detach() for o in out[:5]]).cpu(), 'gaze': out[5].cpu(), 'pupil': out[6].cpu(), 'hs': out[7].cpu(),
           'd_feats': x.grad.cpu(), 'grads': [p.grad.detach().cpu().clone() for p in params]}
    tail_ids = {id(p) for p in params}
    assert all(float(p.grad.abs().max()) == 0 for p in net.parameters() if id(p) not in tail_ids), 'a trunk gradient was written'
    args = (feats, hl, hr, tgt, c_ang, c_l1, B, T)
    want, base = R.tail_f64(sd, *args), R.tail_f32(sd, *args)
    if B * T >= 15 and not right_invalid:
        assert float(want['pupil'].max()) > 0 and float(want['pupil'].min()) == 0         # both sides of the pupil head's ReLU
    worst = []
    for (n, g), (_, w), (_, b), (_, tol) in zip(R.node_tensors(got), R.node_tensors(want), R.node_tensors(base), R.node_tolerances(want, base)):
        assert g.shape == w.shape, (n, g.shape, w.shape)
        assert bool(torch.isfinite(g).all()), n + ': not finite'
        err, dev = float((g.double() - w).abs().max()), float((b.double() - w).abs().max())
        print('B%d T%d%s %-26s err %.3e  float32 chain %.3e  max|want| %.3e  tol %.3e  err/tol %.3f' % (
            B, T, ' R-' if right_invalid else '', n, err, dev, float(w.abs().max()), tol, err / tol))
        worst.append((n, err, tol))
    bad = [(n, err, tol) for n, err, tol in worst if err > tol]
    assert not bad, 'B%d T%d: %s' % (B, T, ', '.join('%s err %.3e > tol %.3e' % t for t in bad))
    if right_invalid:
        BT = B * T
        assert float(got['terms'][2]) == 0 and float(got['terms'][3]) == 0 and float(got['d_feats'][BT:].abs().max()) == 0
