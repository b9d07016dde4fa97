"""float64 references for EyeNet's recurrent scans (eve_amd/csrc/recurrent.hip, recurrent_wide.hip, the autograd shells
GRUScanFn / RNNScanFn / LSTMScanFn of eve_amd/ops.py) and for the conv-RNN gate kernels, with the comparison helpers that
tests/test_gpu_recurrent_cells.py runs on the HIP kernels and tests/test_recurrent_ref_host.py runs on FakeKernels.  CPU only.

  * cell_scan_f64: the real torch.nn.GRUCell / RNNCell / LSTMCell in float64, unrolled over T, differentiated by autograd.
    weight_ih is the identity and bias_ih zero, so the cell's input projection IS gi; no formula of the kernels is restated.
  * restatement_f64: a float64 restatement, used ONLY for the saved intermediates the nn cells do not expose (gates, hn_pre,
    the GRU's dgh); the host test pins its hs / cs / gradients to cell_scan_f64 to 1e-12.
  * gate kernels: the forward formulas of the reference project's CGRUCell / CLSTMCell (common.py:355-415) in float64; every
    backward is autograd of that forward.  A kernel that is handed a stored activation (ru, o) instead of its pre-activation is
    differentiated at the pre-activation that produces exactly that stored value (logit / atanh of it).
  * the helpers take "an object with the gru_scan_fwd ... interface" (HipKernels or FakeKernels) and a `put` that moves a
    tensor to where that object computes.

Tolerances: close() of tests/test_gpu_kernels.py, unchanged (float32: 3e-5 x max|want| and 2e-5 relative L2), against float64;
dW_hh / db_hh by the bound test_small_linear_kernels holds linear_wgrad to (rtol 2e-4, atol 2e-4 sqrt(S T)).
"""
import functools

import torch

from test_gpu_kernels import close

F64 = torch.float64
G_OF = {'gru': 3, 'rnn': 1, 'lstm': 4}
KINDS = ('gru', 'rnn', 'lstm')

# ------------------------------------------------------------------------------------------------ the grid of cases
NARROW_H = (1, 3, 63, 65, 128, 200, 255, 256)      # 1; not a multiple of 4; either side of a wave; register-resident; largest
NARROW_ST = ((1, 1), (3, 2), (3, 30))              # no prefetch at all; one prefetched step; the configured clip length
LONG_CASES = tuple((H, 2, 120) for H in (128, 256))                # streaming length
MANY_CASES = tuple((H, 300, 3) for H in (128, 96))                 # more workgroups than the device has CUs
WIDE_CASES = tuple((H, 17, T) for H in (272, 1024) for T in (1, 2, 30))   # one full tile of 16 sequences plus one row
SAT_CASES = tuple((H, 3, 8) for H in (65, 128, 272))
SHELL_CASES = tuple((H, S, T) for H in (65, 128, 272) for (S, T) in ((3, 5), (2, 30)))
SAT_SCALE = 12.0                                   # test_recurrent_ref_host.py holds the saturation conditions at this scale


def variants(kind):
    """(initial state given, dcs given): GRU / RNN with and without h0; LSTM also with dcs and no initial state and the reverse."""
    if kind == 'lstm':
        return ((False, False), (True, True), (False, True), (True, False))
    return ((False, False), (True, False))


def scan_grid():
    """Every kernel-level case: (kind, H, S, T, variants).  Narrow cases run their variants in one test; the wide ones, whose
    float64 reference is the slow part, one variant a test."""
    narrow = [(H, S, T) for H in NARROW_H for (S, T) in NARROW_ST] + list(LONG_CASES) + list(MANY_CASES)
    grid = [(kind,) + s + (variants(kind),) for kind in KINDS for s in narrow]
    return grid + [(kind,) + s + ((v,),) for kind in KINDS for s in WIDE_CASES for v in variants(kind)]


def grid_id(case):
    kind, H, S, T, vs = case
    tag = '' if len(vs) > 1 else '-' + ('h0' if vs[0][0] else 'no_h0') + ('-dcs' if vs[0][1] else '')
    return '%s-H%d-S%d-T%d%s' % (kind, H, S, T, tag)


def family(H):
    """Which kernel serves the width (decided by H alone; see eve_gru_scan_fwd and its siblings)."""
    return 'wide' if H > 256 else 'narrow-h128' if H == 128 else 'narrow-generic'


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def make_case(kind, H, S, T, with0, with_dcs, scale=1.0, plant=False):
    """float32 operands as the existing scan tests draw them: gi ~ scale N(0, 1), W_hh ~ N(0, 1/H), b ~ 0.1 N, h0, c0 ~ 0.5 N.
    plant: entries of gi set to +-100 and +-1e4 in every gate block (e^x overflows float32 in both directions)."""
    G = G_OF[kind]
    seed = 1000 * G + 7 * H + 3 * S + T
    c = dict(kind=kind, H=H, S=S, T=T,
             gi=rnd((S, T, G * H), seed, scale), whh=rnd((G * H, H), seed + 1, H ** -0.5), bhh=rnd((G * H,), seed + 2, 0.1),
             h0=rnd((S, H), seed + 3, 0.5) if with0 else None,
             c0=rnd((S, H), seed + 4, 0.5) if with0 and kind == 'lstm' else None,
             dhs=rnd((S, T, H), seed + 5), dcs=rnd((S, T, H), seed + 6) if with_dcs else None)
    if plant:
        g = torch.Generator().manual_seed(seed + 7)
        for b in range(G):
            for v in (100.0, -100.0, 1e4, -1e4):
                for _ in range(2):
                    s, t, j = (int(torch.randint(0, n, (1,), generator=g)) for n in (S, T, H))
                    c['gi'][s, t, b * H + j] = v
    return c


def case_name(c):
    return '%s H%d S%d T%d %s%s' % (c['kind'], c['H'], c['S'], c['T'], 'h0' if c['h0'] is not None else 'no-h0',
                                    ' dcs' if c['dcs'] is not None else '')


# ------------------------------------------------------------------------------------------------ nn cells, float64
def d(t):
    return None if t is None else t.detach().to(F64)


def cell_scan_f64(kind, gi, whh, bhh, h0, c0, dhs, dcs):
    """torch.nn cells in float64 over T; the gradients of sum(hs dhs) (+ sum(cs dcs)) by autograd.
    -> dict(hs, cs, dgi, dwhh, dbhh, dh0, dc0); entries that do not exist for the kind / the arguments are None."""
    G = G_OF[kind]
    S, T, GH = gi.shape
    H = GH // G
    cell = {'gru': torch.nn.GRUCell, 'rnn': torch.nn.RNNCell, 'lstm': torch.nn.LSTMCell}[kind](GH, H, dtype=F64)
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(GH, dtype=F64))
        cell.bias_ih.zero_()
        cell.weight_hh.copy_(d(whh))
        cell.bias_hh.copy_(d(bhh))
    cell.weight_ih.requires_grad_(False)
    cell.bias_ih.requires_grad_(False)
    x = d(gi).requires_grad_(True)
    h_init = d(h0).requires_grad_(True) if h0 is not None else None
    c_init = d(c0).requires_grad_(True) if c0 is not None else None
    h = h_init if h_init is not None else torch.zeros((S, H), dtype=F64)
    c = c_init if c_init is not None else torch.zeros((S, H), dtype=F64)
    hs, cs = [], []
    for t in range(T):
        if kind == 'lstm':
            h, c = cell(x[:, t], (h, c))
            cs.append(c)
        else:
            h = cell(x[:, t], h)
        hs.append(h)
    hs = torch.stack(hs, 1)
    cs = torch.stack(cs, 1) if kind == 'lstm' else None
    loss = (hs * d(dhs)).sum() if dhs is not None else 0
    if dcs is not None:
        loss = loss + (cs * d(dcs)).sum()
    wanted = [('dgi', x), ('dwhh', cell.weight_hh), ('dbhh', cell.bias_hh), ('dh0', h_init), ('dc0', c_init)]
    grads = torch.autograd.grad(loss, [t for _, t in wanted if t is not None], allow_unused=True)
    out = dict(hs=hs.detach(), cs=None if cs is None else cs.detach(), dgi=None, dwhh=None, dbhh=None, dh0=None, dc0=None)
    for (name, leaf), g in zip([w for w in wanted if w[1] is not None], grads):
        out[name] = g if g is not None else torch.zeros_like(leaf)
    return out


def restatement_f64(kind, gi, whh, bhh, h0, c0, dhs, dcs):
    """The cells written out in float64, for what nn does not expose: gates [S, T, G H] (GRU r, z, n; LSTM i, f, g, o),
    hn_pre [S, T, H] (the n-block of W_hh h + b_hh) and dgh (the gradient on W_hh h + b_hh: dgi with its n-block times r).
    Gradients by autograd of this forward; pinned to cell_scan_f64 by the host test."""
    G = G_OF[kind]
    S, T, GH = gi.shape
    H = GH // G
    x, w, b = d(gi).requires_grad_(True), d(whh).requires_grad_(True), d(bhh).requires_grad_(True)
    h_init = d(h0).requires_grad_(True) if h0 is not None else None
    c_init = d(c0).requires_grad_(True) if c0 is not None else None
    h = h_init if h_init is not None else torch.zeros((S, H), dtype=F64)
    c = c_init if c_init is not None else torch.zeros((S, H), dtype=F64)
    hs, cs, gates, hn_pre, ghs = [], [], [], [], []
    for t in range(T):
        gh = h @ w.t() + b
        ghs.append(gh)
        if kind == 'gru':
            r = torch.sigmoid(x[:, t, :H] + gh[:, :H])
            z = torch.sigmoid(x[:, t, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(x[:, t, 2 * H:] + r * gh[:, 2 * H:])
            h = (1 - z) * n + z * h
            gates.append(torch.cat([r, z, n], 1)); hn_pre.append(gh[:, 2 * H:])
        elif kind == 'rnn':
            h = torch.tanh(x[:, t] + gh)
        else:
            pre = x[:, t] + gh
            i, f, g, o = (torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]),
                          torch.sigmoid(pre[:, 3 * H:]))
            c = f * c + i * g
            h = o * torch.tanh(c)
            cs.append(c); gates.append(torch.cat([i, f, g, o], 1))
        hs.append(h)
    hs = torch.stack(hs, 1)
    cs = torch.stack(cs, 1) if kind == 'lstm' else None
    loss = (hs * d(dhs)).sum() if dhs is not None else 0
    if dcs is not None:
        loss = loss + (cs * d(dcs)).sum()
    wanted = [('dgi', x), ('dwhh', w), ('dbhh', b), ('dh0', h_init), ('dc0', c_init)] + [('dgh%d' % t, ghs[t]) for t in range(T)]
    wanted = [(n_, t_) for n_, t_ in wanted if t_ is not None]
    grads = dict(zip([n_ for n_, _ in wanted], torch.autograd.grad(loss, [t_ for _, t_ in wanted], allow_unused=True)))
    zero = lambda shape: torch.zeros(shape, dtype=F64)
    out = dict(hs=hs.detach(), cs=None if cs is None else cs.detach(),
               gates=torch.stack(gates, 1).detach() if gates else None,
               hn_pre=torch.stack(hn_pre, 1).detach() if hn_pre else None,
               dgh=torch.stack([grads['dgh%d' % t] if grads['dgh%d' % t] is not None else zero((S, GH)) for t in range(T)], 1))
    for n_ in ('dgi', 'dwhh', 'dbhh', 'dh0', 'dc0'):
        out[n_] = grads.get(n_)
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, H, S, T, with0, with_dcs, scale, plant):
    c = make_case(kind, H, S, T, with0, with_dcs, scale, plant)
    want = cell_scan_f64(kind, c['gi'], c['whh'], c['bhh'], c['h0'], c['c0'], c['dhs'], c['dcs'])
    rs = restatement_f64(kind, c['gi'], c['whh'], c['bhh'], c['h0'], c['c0'], c['dhs'], c['dcs'])
    want.update(gates=rs['gates'], hn_pre=rs['hn_pre'], dgh=rs['dgh'] if kind == 'gru' else None)
    return c, want, rs


def reference(kind, H, S, T, with0, with_dcs, scale=1.0, plant=False):
    """(operands, float64 reference, the float64 restatement): computed once per case, shared, never modified."""
    return _reference(kind, H, S, T, bool(with0), bool(with_dcs), float(scale), bool(plant))


# ------------------------------------------------------------------------------------------------ the chain, kernel level
def run_chain(k, c, put, forward_from=None):
    """k's forward, then k's backward ON THE TENSORS ITS FORWARD STORED -> dict of CPU tensors named as in the reference
    (dpre of the RNN / LSTM under 'dgi').  forward_from: a reference dict whose float32-rounded forward tensors feed the
    backward instead, so that a forward error cannot mask a backward one."""
    kind, with0 = c['kind'], c['h0'] is not None
    gi, whh, bhh, h0, c0, dhs, dcs = (None if c[n] is None else put(c[n]) for n in ('gi', 'whh', 'bhh', 'h0', 'c0', 'dhs', 'dcs'))
    whh_t = whh.t().contiguous()
    f32 = lambda name: put(forward_from[name].float())
    out = {}
    if kind == 'gru':
        hs, gates, hn_pre = k.gru_scan_fwd(gi, whh_t, bhh, h0) if forward_from is None else (f32('hs'), f32('gates'), f32('hn_pre'))
        out.update(hs=hs, gates=gates, hn_pre=hn_pre)
        out['dgi'], out['dgh'], out['dh0'] = k.gru_scan_bwd(dhs, whh, h0, hs, gates, hn_pre, with0)
    elif kind == 'rnn':
        hs = k.rnn_scan_fwd(gi, whh_t, bhh, h0) if forward_from is None else f32('hs')
        out.update(hs=hs)
        out['dgi'], out['dh0'] = k.rnn_scan_bwd(dhs, whh, hs, with0)
    else:
        hs, cs, gates = k.lstm_scan_fwd(gi, whh_t, bhh, h0, c0) if forward_from is None else (f32('hs'), f32('cs'), f32('gates'))
        out.update(hs=hs, cs=cs, gates=gates)
        out['dgi'], out['dh0'], out['dc0'] = k.lstm_scan_bwd(dhs, dcs, whh, c0, hs, cs, gates, with0)
    return {n: (None if t is None else t.detach().cpu()) for n, t in out.items()}


FORWARD_NAMES = ('hs', 'cs', 'gates', 'hn_pre')
BACKWARD_NAMES = ('dgi', 'dgh', 'dh0', 'dc0')


def errors(got, want, names):
    """max|got - float64| / max|float64| per tensor."""
    e = {}
    for n in names:
        if want.get(n) is not None and got.get(n) is not None:
            e[n] = float((got[n].to(F64) - want[n]).abs().max()) / max(float(want[n].abs().max()), 1e-30)
    return e


def compare_chain(got, want, c, names, what):
    """Every tensor of `names` against float64 by close(); no initial state -> no initial-state gradient; the r / z blocks of the
    GRU's dgh are dgi bit for bit (one value stored twice), its n-block is compared against float64 with the rest."""
    H = c['H']
    for n in names:
        if n not in got:
            continue
        if n in ('dh0', 'dc0') and c['h0'] is None:
            assert got[n] is None, '%s: %s without an initial state' % (what, n)
            continue
        assert want[n] is not None and got[n] is not None, '%s: %s missing' % (what, n)
        close(got[n], want[n], torch.float32, '%s %s' % (what, n))
    if c['kind'] == 'gru' and 'dgh' in names:
        assert torch.equal(got['dgh'][..., :2 * H], got['dgi'][..., :2 * H]), '%s: dgh r / z blocks are not dgi' % what
        close(got['dgh'][..., 2 * H:], want['dgh'][..., 2 * H:], torch.float32, '%s dgh n-block' % what)


def check_chain(k, case, put, baseline=None, record=None, tag=''):
    """The whole kernel-level statement for one case = (operands, float64 reference, restatement): forward and backward of `k`
    chained, then the backward alone on the float64-rounded forward tensors.  Prints the error of `k` against float64 per
    tensor; with `baseline` (FakeKernels, on the CPU) also the ratio of the two errors, the restatement's error floored at
    half a float32 spacing of the tensor's maximum, and keeps the worst ratio per (family + tag, kind) in `record`."""
    c, want, _ = case
    name = case_name(c)
    got = run_chain(k, c, put)
    e = errors(got, want, FORWARD_NAMES + BACKWARD_NAMES)
    line = '%-34s ' % name + ' '.join('%s %.1e' % (n, v) for n, v in e.items())
    if baseline is not None:
        eb = errors(run_chain(baseline, c, lambda t: t), want, FORWARD_NAMES + BACKWARD_NAMES)
        ratio = max(e[n] / max(eb[n], 2.0 ** -24) for n in e)
        line += ' | worst err / restatement err %.2f' % ratio
        if record is not None:
            key = (family(c['H']) + tag, c['kind'])
            record[key] = max(record.get(key, 0.0), ratio)
    print(line)
    compare_chain(got, want, c, FORWARD_NAMES + BACKWARD_NAMES, name)
    got2 = run_chain(k, c, put, forward_from=want)
    compare_chain(got2, want, c, BACKWARD_NAMES, name + ' (backward on the float64 forward)')
    return e


# ------------------------------------------------------------------------------------------------ the autograd shells
SHELL_VARIANTS = ('all', 'no-h0', 'bias-only', 'cs-only')


def check_shell(c, want, device, variant='all'):
    """ops.GRUScanFn / RNNScanFn / LSTMScanFn on leaf tensors on `device`, under the process's default kernels, against
    cell_scan_f64 for gi, w_hh, b_hh, h0, c0.  `c` / `want` must fit the variant: 'no-h0' a case without initial state,
    'cs-only' (LSTM) a reference whose loss is sum(cs dcs) alone, 'bias-only' w_hh.requires_grad = False."""
    from eve_amd import ops
    kind, S, T = c['kind'], c['S'], c['T']
    leaf = lambda t, rg=True: None if t is None else t.clone().to(device).requires_grad_(rg)
    gi, whh, bhh, h0, c0 = leaf(c['gi']), leaf(c['whh'], variant != 'bias-only'), leaf(c['bhh']), leaf(c['h0']), leaf(c['c0'])
    assert (variant == 'no-h0') == (h0 is None)
    if kind == 'gru':
        hs, cs = ops.GRUScanFn.apply(gi, whh, bhh, h0), None
    elif kind == 'rnn':
        hs, cs = ops.RNNScanFn.apply(gi, whh, bhh, h0), None
    else:
        hs, cs = ops.LSTMScanFn.apply(gi, whh, bhh, h0, c0)
    what = '%s shell %s' % (case_name(c), variant)
    close(hs, want['hs'], torch.float32, what + ' hs')
    loss = 0
    if variant != 'cs-only':
        loss = (hs * c['dhs'].to(device)).sum()
    if c['dcs'] is not None:
        close(cs, want['cs'], torch.float32, what + ' cs')
        loss = loss + (cs * c['dcs'].to(device)).sum()
    loss.backward()
    close(gi.grad, want['dgi'], torch.float32, what + ' dgi')
    if h0 is not None:
        close(h0.grad, want['dh0'], torch.float32, what + ' dh0')
    if c0 is not None:
        close(c0.grad, want['dc0'], torch.float32, what + ' dc0')
    atol = 2e-4 * (S * T) ** 0.5
    if variant == 'bias-only':
        assert whh.grad is None
    else:
        err = (whh.grad.cpu().to(F64) - want['dwhh']).abs()
        assert bool((err <= atol + 2e-4 * want['dwhh'].abs()).all()), '%s dW_hh: max|diff| %.3e' % (what, float(err.max()))
    err = (bhh.grad.cpu().to(F64) - want['dbhh']).abs()
    assert bool((err <= atol + 2e-4 * want['dbhh'].abs()).all()), '%s db_hh: max|diff| %.3e' % (what, float(err.max()))


@functools.lru_cache(maxsize=None)
def shell_reference(kind, H, S, T, variant):
    with0 = variant != 'no-h0'
    c = make_case(kind, H, S, T, with0, kind == 'lstm')
    want = cell_scan_f64(kind, c['gi'], c['whh'], c['bhh'], c['h0'], c['c0'], None if variant == 'cs-only' else c['dhs'], c['dcs'])
    return c, want


def shell_variants(kind):
    return SHELL_VARIANTS if kind == 'lstm' else SHELL_VARIANTS[:3]


# ------------------------------------------------------------------------------------------------ the conv-RNN gate kernels
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}
GRID_CAP_ITEMS = 2048 * 256                        # rgrid() of recurrent.hip: at most 2048 workgroups of 256 items a turn


def gate_cases(dtype):
    """(P, C, plant): the smallest legal C (one vector); C = 24; one launch whose P C / vec items just exceed the grid cap, so
    that the grid-stride loop takes a second turn; one case with planted saturating gate inputs."""
    vec = VEC[dtype]
    c_cap = 256 if dtype == torch.float32 else 512
    p_cap = GRID_CAP_ITEMS * vec // c_cap + 8
    assert p_cap * (c_cap // vec) > GRID_CAP_ITEMS >= (p_cap - 9) * (c_cap // vec)
    return [(37, vec, False), (41, 24, False), (p_cap, c_cap, False), (45, 24, True)]


def gate_operands(P, C, dtype, plant, seed=0):
    """Operands of the six gate kernels, pre-rounded to `dtype`.  plant: +-100 and +-(1e4, or the largest finite float16)
    written into every gate block of the pre-activations."""
    big = 1e4 if dtype != torch.float16 else float(torch.finfo(torch.float16).max)
    g = torch.Generator().manual_seed(4242 + seed)

    def pre(blocks, sd):
        t = rnd((P, blocks * C), 500 + sd + seed)
        if plant:
            for b in range(blocks):
                for v in (100.0, -100.0, big, -big):
                    for rep in range(3):
                        t[int(torch.randint(0, P, (1,), generator=g)), b * C + int(torch.randint(0, C, (1,), generator=g))] = v
        return t.to(dtype)
    o = dict(g1=pre(2, 1), g2=pre(1, 2), g4=pre(4, 3))
    for i, n in enumerate(('h', 'c_prev')):
        o[n] = rnd((P, C), 510 + i + seed, 0.5).to(dtype)
    for i, n in enumerate(('dhnew', 'drh', 'dh', 'dc_in')):
        o[n] = rnd((P, C), 520 + i + seed).to(dtype)
    o['dru'] = rnd((P, 2 * C), 530 + seed).to(dtype)
    return o


def _leaf(t):
    return t.detach().to(F64).requires_grad_(True)


def _grads(loss, leaves):
    return [g if g is not None else torch.zeros_like(t) for g, t in zip(torch.autograd.grad(loss, leaves, allow_unused=True), leaves)]


def cgru_gates1_f64(g1, h):
    """common.py:409-411: (reset, update) = sigmoid(gates_1); reset * hidden -> ru [P, 2C], rh [P, C]"""
    C = h.shape[-1]
    ru = torch.sigmoid(g1.to(F64))
    return ru, ru[..., :C] * h.to(F64)


def cgru_gates2_f64(g2, ru, h):
    """common.py:413-414: output = tanh(gate_2); hidden = (1 - update) output + update hidden -> o, hnew"""
    C = h.shape[-1]
    o = torch.tanh(g2.to(F64))
    u = ru.to(F64)[..., C:]
    return o, (1 - u) * o + u * h.to(F64)


def cgru_gates2_bwd_f64(dhnew, ru, h, o):
    """autograd of cgru_gates2_f64 at the pre-activation atanh(o) of the stored o -> dg2, dru (its reset half is zero: hnew does
    not read the reset gate), dh (the direct path)"""
    g2, ru_, h_ = _leaf(torch.atanh(o.to(F64))), _leaf(ru), _leaf(h)
    _, hnew = cgru_gates2_f64(g2, ru_, h_)
    return _grads((hnew * dhnew.to(F64)).sum(), [g2, ru_, h_])


def cgru_gates1_bwd_f64(drh, dru, ru, h):
    """autograd of cgru_gates1_f64 at the pre-activation logit(ru) of the stored gates -> dg1, dh.  Upstream: drh on reset *
    hidden and the UPDATE half of dru (the reset gate reaches the step's output through rh alone: cgru_gates2_bwd's reset half
    is zero, and the kernel does not read it)."""
    C = h.shape[-1]
    ruf = ru.to(F64)
    g1, h_ = _leaf(torch.log(ruf) - torch.log1p(-ruf)), _leaf(h)
    ru_, rh = cgru_gates1_f64(g1, h_)
    return _grads((rh * drh.to(F64)).sum() + (ru_[..., C:] * dru.to(F64)[..., C:]).sum(), [g1, h_])


def clstm_gates_f64(g4, c_prev):
    """common.py:376-385: gate order in, forget, out, cell -> hidden, cell"""
    i, f, o, g = g4.to(F64).chunk(4, dim=-1)
    c = torch.sigmoid(f) * c_prev.to(F64) + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def clstm_gates_bwd_f64(dh, dc_in, g4, c_prev):
    """autograd of clstm_gates_f64 -> dgates [P, 4C] (same block order), dc_prev"""
    g_, cp = _leaf(g4), _leaf(c_prev)
    h, c = clstm_gates_f64(g_, cp)
    loss = (h * dh.to(F64)).sum()
    if dc_in is not None:
        loss = loss + (c * dc_in.to(F64)).sum()
    return _grads(loss, [g_, cp])


def check_gates(k, P, C, dtype, plant, put):
    """The six gate kernels of `k` against float64 at one shape, chained the way a step chains them (gates2 reads the ru that
    gates1 stored; each backward reads the stored activations of ITS forward, rounded to `dtype` on both sides)."""
    o = gate_operands(P, C, dtype, plant)
    what = 'P%d C%d %s%s ' % (P, C, str(dtype).split('.')[-1], ' planted' if plant else '')
    p = {n: put(t) for n, t in o.items()}
    ru, rh = k.cgru_gates1(p['g1'], p['h'])
    ru_w, rh_w = cgru_gates1_f64(o['g1'], o['h'])
    close(ru, ru_w, dtype, what + 'gates1 ru')
    close(rh, rh_w, dtype, what + 'gates1 rh')
    ru_s = ru_w.to(dtype)                                            # the stored gates, as a correct forward rounds them
    og, hnew = k.cgru_gates2(p['g2'], put(ru_s), p['h'])
    o_w, hnew_w = cgru_gates2_f64(o['g2'], ru_s, o['h'])
    close(og, o_w, dtype, what + 'gates2 o')
    close(hnew, hnew_w, dtype, what + 'gates2 hnew')
    o_s = o_w.to(dtype)
    for a, b, nm in zip(k.cgru_gates2_bwd(p['dhnew'], put(ru_s), p['h'], put(o_s)),
                        cgru_gates2_bwd_f64(o['dhnew'], ru_s, o['h'], o_s), ('dg2', 'dru', 'dh')):
        close(a, b, dtype, what + 'gates2 bwd ' + nm)
    for a, b, nm in zip(k.cgru_gates1_bwd(p['drh'], p['dru'], put(ru_s), p['h']),
                        cgru_gates1_bwd_f64(o['drh'], o['dru'], ru_s, o['h']), ('dg1', 'dh')):
        close(a, b, dtype, what + 'gates1 bwd ' + nm)
    h, c = k.clstm_gates_fwd(p['g4'], p['c_prev'])
    h_w, c_w = clstm_gates_f64(o['g4'], o['c_prev'])
    close(h, h_w, dtype, what + 'clstm h')
    close(c, c_w, dtype, what + 'clstm c')
    for dc_in in (None, 'dc_in'):
        got = k.clstm_gates_bwd(p['dh'], None if dc_in is None else p[dc_in], p['g4'], p['c_prev'])
        want = clstm_gates_bwd_f64(o['dh'], None if dc_in is None else o[dc_in], o['g4'], o['c_prev'])
        for a, b, nm in zip(got, want, ('dgates', 'dc_prev')):
            close(a, b, dtype, what + 'clstm bwd %s%s' % (nm, '' if dc_in is None else ' with dc_in'))
