"""float64 references of the EyeNet train step's tail node (ops.EyeTailLossFn) and of the kernels only it launches: the batched
weight gradient (linear_wgrad_batch_kernel), the three copy-and-scale kernels around the heads (tail_head_pose, tail_outputs_fwd,
tail_outputs_bwd) and sum_rows_pairs.  Plain torch on the CPU; tests/test_tail_ref_host.py pins this module, and
tests/test_gpu_tail_node.py holds the kernels to it.

A weight-gradient PROBLEM is the dict eve_amd.kernels.HipKernels.linear_wgrad_batch takes -- dY [M, >= N], Y (or None) + act,
X [M, >= K1], K1, X2 [M, K2] (or None), x_shift_T, dW [N, K], db [N] (or None) -- with CPU tensors; dW / db hold the values the
kernel accumulates ONTO.

The arithmetic bound (the argument of wgrad_within_the_arithmetic_bound in tests/test_gpu_kernels.py, with the operands float32
instead of 16 bits wide):  dW[n][k] = base + sum_m G[m][n] Xeff[m][k], G = dY act'(Y).  Any float32 algorithm rounds each product
once and makes M - 1 additions in some order, each off by at most 2^-24 of a partial sum that mag = sum_m |dY| c_act |Xeff| bounds
(c_act = max |act'|); forming G costs a few more roundings of the same relative size (act' from y: two fused multiply-adds, the
product with dY); the sum lands on `base` with one rounding of the total, and the float64 value itself is known to the same
relative precision:
    |err| <= (M + 8) 2^-24 mag + half_ulp32(base) + 2^-24 |want|.
Nothing in it is measured on the code under test.
"""
import math

import torch

F64 = torch.float64
EPS = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SELU, ACT_TANH, ACT_SIGMOID = range(6)       # include/eve_hip.h EVE_ACT_*
SELU_SCALE, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772
WGRAD_BATCH_MAX = 12                                                            # include/eve_hip.h EVE_WGRAD_BATCH_MAX
# max |act'| over the outputs the activation can produce (sigmoid: y (1 - y) on (0, 1))
C_ACT = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_LEAKY: 1.0, ACT_SELU: SELU_SCALE * SELU_ALPHA, ACT_TANH: 1.0, ACT_SIGMOID: 0.25}


def half_ulp32(v):
    """Half the float32 spacing at |v| (0 at 0), as float64."""
    v = v.detach().cpu().float()
    _, e = torch.frexp(v.abs())                                 # |v| = m 2^e, m in [0.5, 1): ulp = 2^(e - 24)
    return torch.where(v == 0, torch.zeros((), dtype=F64), torch.ldexp(torch.ones((), dtype=F64), e - 25))


def ulp32(v):
    return 2.0 * half_ulp32(v)


# ------------------------------------------------------------------------------------------------ activations
def act_fwd(z, act):
    """The activation itself (to make a Y that lies in its range)."""
    if act == ACT_RELU:
        return z.clamp(min=0)
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, 0.01 * z)
    if act == ACT_SELU:
        return SELU_SCALE * torch.where(z > 0, z, SELU_ALPHA * torch.expm1(z))
    if act == ACT_TANH:
        return torch.tanh(z)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    return z


def act_grad_from_out(y, act):
    """act'(.) restated from the STORED output y, as the kernels read it (lm_act_grad in csrc/linear_small.hip)."""
    one = torch.ones_like(y)
    if act == ACT_RELU:
        return torch.where(y > 0, one, 0 * one)
    if act == ACT_LEAKY:
        return torch.where(y > 0, one, 0.01 * one)
    if act == ACT_SELU:
        return torch.where(y > 0, SELU_SCALE * one, y + SELU_SCALE * SELU_ALPHA)
    if act == ACT_TANH:
        return 1 - y * y
    if act == ACT_SIGMOID:
        return y - y * y
    return one


# ------------------------------------------------------------------------------------------------ the batched weight gradient
def problem_dims(p):
    """-> M, N, K, K1, K2"""
    N, K = p['dW'].shape
    K2 = p['X2'].shape[1] if p.get('X2') is not None else 0
    return p['dY'].shape[0], N, K, p.get('K1', p['X'].shape[1]), K2


def effective_x(p, dtype=F64, zero_first_step=True):
    """[M, K]: the leading K1 columns of X, then X2, then zeros up to K; under x_shift_T = T row m - 1 of X, zero where m % T == 0.
    zero_first_step = False plants the defect of a shift that runs across the sequence boundary (row 0 stays zero)."""
    M, N, K, K1, K2 = problem_dims(p)
    x = torch.zeros((M, K), dtype=dtype)
    T = int(p.get('x_shift_T', 0) or 0)
    if T:
        assert K2 == 0 and K1 == K and M % T == 0
        x[1:] = p['X'][:-1, :K].to(dtype)
        if zero_first_step:
            x[::T] = 0
        return x
    x[:, :K1] = p['X'][:, :K1].to(dtype)
    if K2:
        x[:, K1:K1 + K2] = p['X2'].to(dtype)
    return x


def wgrad_g(p, dtype=F64):
    M, N, K, K1, K2 = problem_dims(p)
    g = p['dY'][:, :N].to(dtype)
    act = p.get('act', ACT_NONE) if p.get('Y') is not None else ACT_NONE
    if act != ACT_NONE:
        g = g * act_grad_from_out(p['Y'][:, :N].to(dtype), act)
    return g, act


def wgrad_batch_f64(p, zero_first_step=True, drop_last_row=False):
    """One problem in float64 -> {'dW', 'db' (None without db), 'mag_W', 'mag_b', 'bound_W', 'bound_b'}.
    drop_last_row plants the defect of a ragged last split that loses its last row."""
    M, N, K, K1, K2 = problem_dims(p)
    g, act = wgrad_g(p)
    x = effective_x(p, F64, zero_first_step)
    if drop_last_row:
        g, x = g[:-1], x[:-1]
    ga = p['dY'][:, :N].to(F64).abs() * C_ACT[act]
    xa = effective_x(p).abs()
    out = {'dW': p['dW'].to(F64) + g.t() @ x, 'mag_W': ga.t() @ xa, 'db': None, 'mag_b': None, 'bound_b': None}
    out['bound_W'] = (M + 8) * EPS * out['mag_W'] + half_ulp32(p['dW']) + EPS * out['dW'].abs()
    if p.get('db') is not None:
        out['db'] = p['db'].to(F64) + g.sum(0)
        out['mag_b'] = ga.sum(0)
        out['bound_b'] = (M + 8) * EPS * out['mag_b'] + half_ulp32(p['db']) + EPS * out['db'].abs()
    return out


def wgrad_batch_f32_pieces(p, piece=64):
    """The float32 restatement: G and Xeff formed in float32, the sums in 64-row pieces added one after the other onto the base.
    -> dW, db (or None), float32"""
    g, _ = wgrad_g(p, torch.float32)
    x = effective_x(p, torch.float32)
    dw = p['dW'].clone().float()
    db = p['db'].clone().float() if p.get('db') is not None else None
    for m in range(0, g.shape[0], piece):
        dw += g[m:m + piece].t() @ x[m:m + piece]
        if db is not None:
            db += g[m:m + piece].sum(0)
    return dw, db


def bound_ratios(got_w, got_b, ref):
    """max err / bound of a result against wgrad_batch_f64's -> (dW ratio, db ratio or None)"""
    def ratio(got, want, bound):
        err = (got.detach().cpu().to(F64) - want).abs()
        assert bool(torch.isfinite(err).all())
        return float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())
    return ratio(got_w, ref['dW'], ref['bound_W']), (ratio(got_b, ref['db'], ref['bound_b']) if ref['db'] is not None else None)


def expected_splits(problems, batch=True):
    """lm_wgrad_tiles / lm_wgrad_split of csrc/linear_small.hip restated: per problem {'tiles': 32 x 32 tiles of dW, 'rows': rows
    per split (whole 64-row steps), 'sizes': the rows of every split, 'first_block'}.  batch: the split count comes from the tiles
    of ALL problems (eve_linear_wgrad_batch); eve_linear_wgrad counts its one problem's own, which is the same for one problem."""
    dims = [problem_dims(p)[:3] for p in problems]
    tiles = [((K + 31) // 32) * ((N + 31) // 32) for M, N, K in dims]
    total = max(sum(tiles), 1) if batch else None
    out, first = [], 0
    for (M, N, K), t in zip(dims, tiles):
        tt = total if batch else t
        splits = max(1, min((512 + tt // 2) // tt, (M + 63) // 64))
        rows = ((M + splits - 1) // splits + 63) // 64 * 64
        sizes = [min(rows, M - m) for m in range(0, M, rows)]
        out.append({'tiles': t, 'rows': rows, 'sizes': sizes, 'first_block': first})
        first += t * len(sizes)
    return out


# ---- operands
def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g) * scale).float()


def make_problem(M, N, K, seed, act=ACT_NONE, K1=None, K2=0, ldx=None, ldy=None, shift_T=0, db=True, base=True):
    """Random float32 operands: dW / db start from nonzero values (base), Y lies in the activation's range."""
    K1 = K if K1 is None else K1
    p = {'dY': rnd((M, ldy or N), seed), 'X': rnd((M, ldx or K1), seed + 1), 'act': act, 'K1': K1,
         'dW': rnd((N, K), seed + 2, 3.0) if base else torch.zeros((N, K)),
         'db': (rnd((N,), seed + 3, 3.0) if base else torch.zeros((N,))) if db else None}
    if act != ACT_NONE:
        p['Y'] = act_fwd(rnd((M, ldy or N), seed + 4), act)
    if K2:
        p['X2'] = rnd((M, K2), seed + 5)
    if shift_T:
        p['x_shift_T'] = shift_T
    return p


def product_problems(B, T, seed=100, last_n=(4, 4), acts=None):
    """The nine problems of EyeTailLossFn.backward at M = 2 B T rows.  last_n: rows of the two last layers' dW (4, 4: the padded
    layers; 2, 1: the parameters' own shapes, read from 4-wide dY / Y as the node does)."""
    M = 2 * B * T
    mk = lambda i, *a, **kw: make_problem(M, *a, seed=seed + 10 * i, **kw)
    ps = [mk(0, 128, 512),                                            # fc
          mk(1, 128, 130, act=ACT_SELU, K1=130, ldx=132),             # fc_common.0: X is the 132-wide concatenation
          mk(2, 128, 128),                                            # fc_common.2
          mk(3, 384, 128),                                            # GRU W_ih
          mk(4, 384, 128, shift_T=T),                                 # GRU W_hh: X = hs shifted by one step
          mk(5, 128, 128, act=ACT_SELU),                              # gaze head
          mk(6, last_n[0], 128, act=ACT_TANH, ldy=4, db=False),       # its last layer, no bias
          mk(7, 128, 128, act=ACT_SELU),                              # pupil head
          mk(8, last_n[1], 128, act=ACT_RELU, ldy=4)]                 # its last layer
    if acts is not None:                                              # (the exact regime keeps none / ReLU only)
        ps = [p for p in ps if p['act'] in acts]
    return ps


MASKED_MNK = ((5, 3, 7), (65, 4, 130), (33, 17, 33))         # every nok / kok / mok mask of the kernel in play


def full_batch():
    """WGRAD_BATCH_MAX problems of mixed shapes, row counts and activations (every code lm_act_grad accepts) in one call."""
    spec = [(130, 40, 70, ACT_NONE, {}), (65, 4, 130, ACT_RELU, {'ldy': 8}), (33, 17, 33, ACT_LEAKY, {}), (96, 64, 32, ACT_SELU, {'db': False}),
            (200, 33, 65, ACT_TANH, {}), (64, 32, 32, ACT_SIGMOID, {}), (60, 48, 16, ACT_NONE, {'shift_T': 12}), (5, 3, 7, ACT_SELU, {}),
            (128, 96, 40, ACT_NONE, {'K1': 36, 'K2': 3}), (1, 1, 1, ACT_TANH, {}), (77, 20, 100, ACT_RELU, {'K1': 90, 'ldx': 92}),
            (256, 8, 8, ACT_NONE, {'db': False})]
    assert len(spec) == WGRAD_BATCH_MAX
    return [make_problem(M, N, K, 700 + 10 * i, act=a, **kw) for i, (M, N, K, a, kw) in enumerate(spec)]


def bound_cases():
    """name -> problems of one launch: the cases of the arithmetic-bound regime (M <= 480), shared by the CPU and the GPU tests."""
    c = {'shift M130 T13': [make_problem(130, 128, 128, 10, shift_T=13)],
         'product B4 T30': product_problems(4, 30),
         'product B8 T30': product_problems(8, 30),
         'product B4 T30, parameter shapes': product_problems(4, 30, last_n=(2, 1)),
         'X2 128+2': [make_problem(130, 128, 130, 20, K1=128, K2=2)],
         'K1 < K': [make_problem(130, 128, 130, 30, K1=128)],
         'wide dY SELU': [make_problem(100, 60, 64, 40, act=ACT_SELU, ldy=64)],
         'full batch': full_batch()}
    for M, N, K in MASKED_MNK:
        c['masked %dx%dx%d' % (M, N, K)] = [make_problem(M, N, K, 50 + M, act=ACT_TANH)]
    return c


def exactify(p, seed):
    """The same problem on integer-valued operands (exact_conv's exact value sets; ReLU reads an integer Y, zeros included):
    every sum stays below 2^24 in magnitude, so float32 accumulation in any order gives the integer."""
    import exact_conv as ec
    assert p.get('act', ACT_NONE) in (ACT_NONE, ACT_RELU)
    q = dict(p)
    q['dY'] = ec.pick(p['dY'].shape, ec.signed([1, 2]), seed)
    q['X'] = ec.pick(p['X'].shape, ec.signed([1]), seed + 1)
    if p.get('X2') is not None:
        q['X2'] = ec.pick(p['X2'].shape, ec.signed([1]), seed + 2)
    if p.get('Y') is not None:
        q['Y'] = ec.pick(p['Y'].shape, [-2.0, -1.0, 0.0, 1.0, 2.0], seed + 3)
    q['dW'] = ec.big_ints(p['dW'].shape, 300, 900, seed + 4)
    if p.get('db') is not None:
        q['db'] = ec.big_ints(p['db'].shape, 300, 900, seed + 5)
    ec.assert_below_2_24(2.0 * p['dY'].shape[0] + 900, 'exact wgrad')
    return q


def exact_cases():
    c = {'shift M130 T13': [make_problem(130, 128, 128, 10, shift_T=13)],
         'product B4 T30, none / ReLU': product_problems(4, 30, acts=(ACT_NONE, ACT_RELU)),
         'M1921 32x32': [make_problem(1921, 32, 32, 60)]}
    return {n: [exactify(p, 900 + 10 * i) for i, p in enumerate(ps)] for n, ps in c.items()}


# ------------------------------------------------------------------------------------------------ the small kernels
def head_pose_f64(cat, h_left, h_right, col):
    """cat [2 BT, ld]: columns col, col + 1 <- the left clips' rows, then the right clips'; col + 2, col + 3 <- 0; the rest kept."""
    out = cat.to(F64).clone()
    out[:, col:col + 2] = torch.cat([h_left.reshape(-1, 2), h_right.reshape(-1, 2)]).to(F64)
    out[:, col + 2:col + 4] = 0
    return out


def outputs_fwd_f64(g2, p2):
    return (math.pi / 2) * g2[:, :2].to(F64), p2[:, 0].to(F64)


def outputs_bwd_f64(dg_l, dg_r, dp_l, dp_r, g_full, c_ang, c_l1):
    """-> d_g2, d_p2 [2 BT, 4]; g_full: None (1) or a scalar tensor"""
    up = 1.0 if g_full is None else float(g_full)
    dg = torch.cat([dg_l.reshape(-1, 2), dg_r.reshape(-1, 2)]).to(F64)
    dp = torch.cat([dp_l.reshape(-1), dp_r.reshape(-1)]).to(F64)
    d_g2, d_p2 = torch.zeros((dg.shape[0], 4), dtype=F64), torch.zeros((dg.shape[0], 4), dtype=F64)
    d_g2[:, :2] = (math.pi / 2) * float(c_ang) * up * dg
    d_p2[:, 0] = float(c_l1) * up * dp
    return d_g2, d_p2


def sum_rows_pairs_f64(sums, out0, out1):
    """sums [rows, C, 2] -> out0 + sums[:, :, 0].sum(0), out1 + sums[:, :, 1].sum(0), and the bound of any float32 summation:
    rows 2^-24 sum |in| + 2^-24 (|want| + |base|)."""
    s = sums.to(F64)
    res = []
    for j, base in enumerate((out0, out1)):
        want = base.to(F64) + s[:, :, j].sum(0)
        res.append((want, s.shape[0] * EPS * s[:, :, j].abs().sum(0) + EPS * (want.abs() + base.to(F64).abs())))
    return res


def sum_rows_pairs_f32(sums, out0, out1):
    """float32, one row after the other"""
    a, b = out0.clone().float(), out1.clone().float()
    acc = torch.zeros_like(sums[0])
    for r in range(sums.shape[0]):
        acc += sums[r]
    return a + acc[:, 0], b + acc[:, 1]


# ------------------------------------------------------------------------------------------------ the whole node
TAIL_KEYS = ('cnn_layers.fc.weight', 'cnn_layers.fc.bias', 'fc_common.0.weight', 'fc_common.0.bias', 'fc_common.2.weight',
             'fc_common.2.bias', 'rnn_cells.0.weight_ih', 'rnn_cells.0.bias_ih', 'rnn_cells.0.weight_hh', 'rnn_cells.0.bias_hh',
             'fc_to_gaze.0.weight', 'fc_to_gaze.0.bias', 'fc_to_gaze.2.weight', 'fc_to_pupil.0.weight', 'fc_to_pupil.0.bias',
             'fc_to_pupil.2.weight', 'fc_to_pupil.2.bias')               # the order of ops.EyeTailLossFn.tail_parameters
TAIL_SHAPES = ((128, 512), (128,), (128, 130), (128,), (128, 128), (128,), (384, 128), (384,), (384, 128), (384,), (128, 128), (128,),
               (2, 128), (128, 128), (128,), (1, 128), (1,))
TERM_NAMES = ('ang_l', 'l1_l', 'ang_r', 'l1_r', 'full')


def random_state_dict(seed):
    """Tail parameters of the module's shapes at the scale of a default nn.Linear (1 / sqrt(fan in)); the pupil head's last layer
    is scaled up so that its ReLU passes most rows and stops some."""
    sd = {k: rnd(s, seed + i, 1.0 / math.sqrt(s[-1]) if len(s) == 2 else 0.05) for i, (k, s) in enumerate(zip(TAIL_KEYS, TAIL_SHAPES))}
    sd['fc_to_pupil.2.weight'] *= 4.0
    return sd


def selu(x):
    return SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(x))


def tail_chain(params, feats, h_left, h_right, B, T):
    """eye_net.py's tail on rows ordered (left clips, right clips) x time, in the dtype of its arguments -> gaze [M, 2], pupil [M],
    hs [2 B, T, 128].  The GRU cell written out (torch.nn.GRUCell's definition), from a zero state."""
    (w_fc, b_fc, w0, b0, w2, b2, w_ih, b_ih, w_hh, b_hh, wg0, bg0, wg2, wp0, bp0, wp2, bp2) = params
    x = feats @ w_fc.t() + b_fc
    x = torch.cat([x, torch.cat([h_left.reshape(-1, 2), h_right.reshape(-1, 2)]).to(x.dtype)], dim=1)
    x = selu(x @ w0.t() + b0) @ w2.t() + b2
    gi = (x @ w_ih.t() + b_ih).view(2 * B, T, 384)
    h = torch.zeros((2 * B, 128), dtype=x.dtype)
    hs = []
    for t in range(T):
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, t, :128] + gh[:, :128])
        z = torch.sigmoid(gi[:, t, 128:256] + gh[:, 128:256])
        n = torch.tanh(gi[:, t, 256:] + r * gh[:, 256:])
        h = (1 - z) * n + z * h
        hs.append(h)
    hs = torch.stack(hs, dim=1)
    f = hs.reshape(2 * B * T, 128)
    gaze = (math.pi / 2) * torch.tanh(selu(f @ wg0.t() + bg0) @ wg2.t())
    pupil = torch.relu(selu(f @ wp0.t() + bp0) @ wp2.t() + bp2)[:, 0]
    return gaze, pupil, hs


def _tail(state_dict, feats, h_left, h_right, targets, c_ang, c_l1, B, T, dtype, eye_terms):
    params = [state_dict[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in TAIL_KEYS]
    x = feats.detach().cpu().to(dtype).clone().requires_grad_(True)
    gaze, pupil, hs = tail_chain(params, x, h_left.detach().cpu().to(dtype), h_right.detach().cpu().to(dtype), B, T)
    BT = B * T
    tg_l, tg_r, vg_l, vg_r, tp_l, tp_r, vp_l, vp_r = [t.detach().cpu() for t in targets]
    gd, pd = gaze.detach(), pupil.detach()
    terms, dg, dp = eye_terms((gd[:BT].view(B, T, 2), gd[BT:].view(B, T, 2)), (tg_l, tg_r), (vg_l, vg_r),
                              (pd[:BT].view(B, T), pd[BT:].view(B, T)), (tp_l, tp_r), (vp_l, vp_r), c_ang, c_l1)
    d_gaze = c_ang * torch.cat([dg[0].reshape(-1, 2), dg[1].reshape(-1, 2)]).to(dtype)
    d_pupil = c_l1 * torch.cat([dp[0].reshape(-1), dp[1].reshape(-1)]).to(dtype)
    grads = torch.autograd.grad([gaze, pupil], [x] + params, [d_gaze, d_pupil])
    return {'terms': terms.detach(), 'gaze': gd, 'pupil': pd, 'hs': hs.detach(), 'd_feats': grads[0], 'grads': list(grads[1:])}


def eye_terms_f64(g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, c_ang, c_l1):
    """The four masked terms, their weighted sum and the unit gradients per side: harness_ref's float64 statement of eye_losses."""
    import harness_ref as hr
    terms, dg, dp = [], [], []
    for s in range(2):
        va, ga, _ = hr.term_f64('angular', g_pred[s], g_tgt[s], g_val[s])
        vl, gl, _ = hr.term_f64('l1', p_pred[s], p_tgt[s], p_val[s])
        terms += [va, vl]
        dg.append(ga); dp.append(gl)
    return torch.stack(terms + [c_ang * (terms[0] + terms[2]) + c_l1 * (terms[1] + terms[3])]), dg, dp


def tail_f64(state_dict, feats, h_left, h_right, targets, c_ang, c_l1, B, T):
    """The whole node in float64 with autograd: {'terms' [5] (ang_l, l1_l, ang_r, l1_r, full), 'gaze' [M, 2], 'pupil' [M],
    'hs' [2 B, T, 128], 'd_feats' [M, 512], 'grads': the 17 gradients of d(full) in TAIL_KEYS order}.
    targets: (g_l, g_r, g validity l, r, pupil l, r, pupil validity l, r) as EyeTailLossFn takes them."""
    return _tail(state_dict, feats, h_left, h_right, targets, c_ang, c_l1, B, T, F64, eye_terms_f64)


def tail_f32(state_dict, feats, h_left, h_right, targets, c_ang, c_l1, B, T):
    """The same chain under float32 autograd on the CPU, the loss terms from harness_ref's float32 restatement: the yardstick
    of the GPU node's deviation from float64."""
    import harness_ref as hr
    return _tail(state_dict, feats, h_left, h_right, targets, c_ang, c_l1, B, T, torch.float32, hr.BASE.eye_losses)


NODE_BT = ((1, 1), (3, 5), (2, 33), (5, 30), (8, 30))


def node_case(B, T, right_invalid=False, seed=0):
    """feats [2 B T, 512], head poses, targets with 25 % invalid steps (right_invalid: the whole right eye invalid)."""
    s = 1000 * seed + 31 * B + T
    g = torch.Generator().manual_seed(s)
    feats = rnd((2 * B * T, 512), s + 1).abs() * 0.7                       # (pooled ReLU features: non-negative)
    h = [rnd((B, T, 2), s + 2 + i, 0.1) for i in range(2)]
    tg = [rnd((B, T, 2), s + 4 + i, 0.2) for i in range(2)]
    tp = [torch.rand((B, T), generator=g) * 4.0 for _ in range(2)]
    val = [torch.rand((B, T), generator=g) >= 0.25 for _ in range(4)]      # g l, g r, p l, p r
    if right_invalid:
        val[1][:] = False
        val[3][:] = False
    return feats, h[0], h[1], (tg[0], tg[1], val[0], val[1], tp[0], tp[1], val[2], val[3])


def node_tensors(res):
    """-> [(name, tensor)] of everything the node is compared on"""
    out = [('term ' + n, res['terms'][i:i + 1]) for i, n in enumerate(TERM_NAMES)]
    out += [('gaze', res['gaze']), ('pupil', res['pupil']), ('hs', res['hs']), ('d_feats', res['d_feats'])]
    return out + [('d ' + k, g) for k, g in zip(TAIL_KEYS, res['grads'])]


def node_tolerances(want, base):
    """Per tensor: max(4 x the float32 restatement's deviation from float64, 1e-6 max(1, max |want|))."""
    return [(n, max(4.0 * float((b.to(F64) - w).abs().max()), 1e-6 * max(1.0, float(w.abs().max()))))
            for (n, w), (_, b) in zip(node_tensors(want), node_tensors(base))]
