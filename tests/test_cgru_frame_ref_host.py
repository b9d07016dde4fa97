"""CPU: the judge of cgru_frame_ref.py against stand-ins of the 16-bit conv-GRU clip scans -- the float32 contract with the
kernels' rounding points must pass at the very inputs test_gpu_cgru_scan_frames.py uses and stay under both caps (so the inputs are
well chosen), and each of nine deliberately wrong stand-ins must fail (so the judge sees what the whole-clip bounds do not)."""
import pytest
import torch

import cgru_frame_ref as cf
import refine_variants as rv

DTYPES = [torch.bfloat16, torch.float16]
dtid = lambda v: str(v).split('.')[-1]


def fwd_standin(xs, h0, w1, b1, w2, b2, rnd, fault=None):
    """contract_cgru_fwd on float32 operands with the storage rounding `rnd`, and one way of being wrong:
    'tap'       one filter element (output channel 5, tap (1, 0), one input channel) dropped at border pixel (0, 3) of sequence 0
    'halo'      sequence 1's first image row used as sequence 0's bottom halo row (gates_1)
    'raw_r'     r * h formed from the unrounded r
    'h_t2'      the blend reads h_{t-2}
    'x_next'    x_{t+1} read in place of x_t at frame 0
    (truncation is a choice of rnd)"""
    B, T, C = xs.shape[0], xs.shape[1], xs.shape[-1]
    h = torch.zeros_like(xs[:, 0]) if h0 is None else h0
    h2 = h
    hs, rus, rhs, ogs = [], [], [], []
    for t in range(T):
        x = xs[:, t + 1] if (fault == 'x_next' and t == 0) else xs[:, t]
        cat1 = torch.cat([x, h], -1)
        pre1 = rv._conv(cat1, w1, b1)
        if fault == 'tap':
            # tap (ky, kx) = (1, 0) of output pixel (0, 3) reads input pixel (0, 2); the input channel is the one whose product is
            # nearest 0.04 * 0.8, the typical size of one
            prod = w1[5, 1, 0, :] * cat1[0, 0, 2, :]
            pre1[0, 0, 3, 5] -= prod[int((prod.abs() - 0.032).abs().argmin())]
        if fault == 'halo':
            tall = torch.cat([cat1[0], cat1[1][:1]], 0)[None]                  # 6 rows: the image, then its wrong bottom halo
            pre1[0] = rv._conv(tall, w1, b1)[0, :5]
        ru_raw = torch.sigmoid(pre1)
        ru = rnd(ru_raw)
        rh = rnd((ru_raw if fault == 'raw_r' else ru)[..., :C] * h)
        o = rnd(torch.tanh(rv._conv(torch.cat([rh, x], -1), w2, b2)))
        u = ru[..., C:]
        new = rnd((1 - u) * o + u * (h2 if fault == 'h_t2' else h))
        h2, h = h, new
        hs.append(h); rus.append(ru); rhs.append(rh); ogs.append(o)
    return torch.stack(hs, 1), torch.stack(hs, 0), torch.stack(rus, 0), torch.stack(rhs, 0), torch.stack(ogs, 0)


def bwd_standin(dhs, ru, og, hs_tm, h0, w1t, w2t, want_dh0, rnd, fault=None):
    """contract_cgru_bwd on float32 operands with the 16-bit scans' rounding points (dg2 and dg1 rounded before their data-gradient
    GEMMs, dxs and dh0 on the way out, the carry in float32), and one way of being wrong:
    'no_drh_r'   the carry without its d(r h) * r term
    'unmirrored' the data gradients walk the taps in the forward's order
    'swapped'    the reset and update halves of dg1 swapped"""
    T, C = dhs.shape[0], dhs.shape[-1]
    if fault == 'unmirrored':
        w1t, w2t = w1t.flip(1, 2), w2t.flip(1, 2)
    carry = torch.zeros_like(dhs[0])
    dg1_all, dg2_all, dxs = [None] * T, [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        hp = hs_tm[t - 1] if t > 0 else (h0 if h0 is not None else torch.zeros_like(hs_tm[0]))
        r, u, o = ru[t][..., :C], ru[t][..., C:], og[t]
        dhn = dhs[t] + carry
        dg2 = rnd(dhn * (1 - u) * (1 - o * o))
        dcat2 = rv._dgrad(dg2, w2t)
        drh, dx2 = dcat2[..., :C], dcat2[..., C:]
        halves = [drh * hp * r * (1 - r), dhn * (hp - o) * u * (1 - u)]
        dg1 = rnd(torch.cat(halves[::-1] if fault == 'swapped' else halves, -1))
        dcat1 = rv._dgrad(dg1, w1t)
        carry = dhn * u + (0 if fault == 'no_drh_r' else drh * r) + dcat1[..., C:]
        dg1_all[t], dg2_all[t], dxs[t] = dg1, dg2, rnd(dcat1[..., :C] + dx2)
    return torch.stack(dg1_all, 0), torch.stack(dg2_all, 0), torch.stack(dxs, 0), (rnd(carry) if want_dh0 else None)


def run_fwd(inp, dt, rnd=None, fault=None, standin=None):
    rnd = rnd or (lambda v: cf.rne(v, dt))
    f = lambda k: None if inp[k] is None else inp[k].float()
    args = (f('xs'), f('h0'), f('w1'), inp['b1'], f('w2'), inp['b2'])
    out = rv.contract_cgru_fwd(*args, rnd=rnd) if standin == 'contract' else fwd_standin(*args, rnd, fault)
    return [t.to(dt) for t in out]


def run_bwd(inp, dt, fault=None):
    f = lambda k: None if inp[k] is None else inp[k].float()
    out = bwd_standin(f('dhs'), f('ru'), f('og'), f('hs_tm'), f('h0'), f('w1t'), f('w2t'), inp['h0'] is not None,
                      lambda v: cf.rne(v, dt), fault)
    return [None if t is None else t.to(dt) for t in out]


def judge_fwd(inp, dt, out, **kw):
    return cf.judge_forward(dt, inp['xs'], inp['h0'], inp['w1'], inp['b1'], inp['w2'], inp['b2'], *out, **kw)


def judge_bwd(inp, dt, out, **kw):
    return cf.judge_backward(dt, inp['dhs'], inp['ru'], inp['og'], inp['hs_tm'], inp['h0'], inp['w1t'], inp['w2t'], *out, **kw)


# ------------------------------------------------------------------------------------------------ the right stand-ins pass
@pytest.mark.parametrize('dt', DTYPES, ids=dtid)
@pytest.mark.parametrize('C', cf.WIDTHS)
def test_the_rounded_float32_contract_passes_at_the_gpu_inputs_and_stays_under_both_caps(C, dt):
    """contract_cgru_fwd(rnd = RNE to the format) and the backward stand-in, at every shape of the GPU cases.  A float32 evaluation
    in ATen's order is what eps is measured on, so the ratios printed here are far below the margin of 8; the caps are the point."""
    for B, T, with_h0 in cf.SHAPES:
        inp = cf.make_inputs(C, B, T, with_h0, dt, cf.seed_of(C, B, T))
        out = run_fwd(inp, dt, standin='contract')
        assert all(torch.equal(a, b) for a, b in zip(out, run_fwd(inp, dt)))           # the faulty stand-ins start from the same thing
        rep = judge_fwd(inp, dt, out)
        print('forward C=%d B=%d T=%d %s: %s' % (C, B, T, dtid(dt), rep.summary()))
        rep.assert_ok('forward')
        rep = judge_bwd(inp, dt, run_bwd(inp, dt))
        print('backward C=%d B=%d T=%d %s: %s' % (C, B, T, dtid(dt), rep.summary()))
        rep.assert_ok('backward')
        if (B, T) == (7, 30):
            # the backward on the tensors a forward stored, as the GPU case runs it
            own = dict(inp, hs_tm=out[1], ru=out[2], og=out[4])
            rep = judge_bwd(own, dt, run_bwd(own, dt))
            print('backward on the forward\'s tensors C=%d %s: %s' % (C, dtid(dt), rep.summary()))
            rep.assert_ok('backward on the forward\'s tensors')


@pytest.mark.parametrize('dt', DTYPES, ids=dtid)
@pytest.mark.parametrize('C', cf.WIDTHS)
def test_saturated_gates_pass_and_reach_the_ends_of_the_format(C, dt):
    """Filters x 8: gates of exactly 1 (and, in float16, exactly 0; bfloat16 has float32's range, there a sigmoid gate gets below
    2^-9 and its complement rounds to 1).  The bound holds; the caps do not apply (a tenth of the float16 gates is subnormal)."""
    inp = cf.make_inputs(C, 4, 2, True, dt, cf.seed_of(C, 4, 2) + 1, gain=8.0)
    out = run_fwd(inp, dt, standin='contract')
    ru, og = out[2].float(), out[4].float()
    assert bool((ru == 1).any()) and bool((og.abs() == 1).any()) and float(ru.min()) < 2.0 ** -9
    assert dt != torch.float16 or bool((ru == 0).any())
    rep = judge_fwd(inp, dt, out, caps=False)
    rep.assert_ok('saturated forward')
    own = dict(inp, hs_tm=out[1], ru=out[2], og=out[4])
    judge_bwd(own, dt, run_bwd(own, dt), caps=False).assert_ok('saturated backward')


# ------------------------------------------------------------------------------------------------ the wrong stand-ins fail
FWD_FAULTS = ['tap', 'halo', 'raw_r', 'h_t2', 'x_next', 'truncation']
BWD_FAULTS = ['no_drh_r', 'unmirrored', 'swapped']


def faulty_fwd(inp, dt, fault):
    if fault == 'truncation':
        return run_fwd(inp, dt, rnd=lambda v: cf.truncate(v, dt))
    return run_fwd(inp, dt, fault=fault)


@pytest.mark.parametrize('dt', DTYPES, ids=dtid)
@pytest.mark.parametrize('fault', FWD_FAULTS)
def test_a_wrong_forward_stand_in_fails(fault, dt):
    inp = cf.make_inputs(64, 5, 3, False, dt, cf.seed_of(64, 5, 3))
    rep = judge_fwd(inp, dt, faulty_fwd(inp, dt, fault))
    print(fault, dtid(dt), rep.failures[:2])
    assert not rep.ok


@pytest.mark.parametrize('dt', DTYPES, ids=dtid)
@pytest.mark.parametrize('fault', BWD_FAULTS)
def test_a_wrong_backward_stand_in_fails(fault, dt):
    inp = cf.make_inputs(64, 5, 3, False, dt, cf.seed_of(64, 5, 3))
    rep = judge_bwd(inp, dt, run_bwd(inp, dt, fault=fault))
    print(fault, dtid(dt), rep.failures[:2])
    assert not rep.ok


def test_the_judge_measures_half_a_unit_of_the_format():
    for dt, (p, emin) in cf.FORMATS.items():
        v = torch.tensor([1.0, 1.5, 0.75, 2.0 ** emin, 2.0 ** (emin - 3), 0.0, -3.0], dtype=torch.float64)
        want = [2.0 ** (1 - p), 2.0 ** (1 - p), 2.0 ** -p, 2.0 ** (emin + 1 - p), 2.0 ** (emin + 1 - p), 2.0 ** (emin + 1 - p), 2.0 ** (2 - p)]
        assert cf.ulp(v, dt).tolist() == want
        x = torch.tensor([1.0 + 0.75 * 2.0 ** (1 - p), -(1.0 + 0.75 * 2.0 ** (1 - p)), 1.0 + 0.25 * 2.0 ** (1 - p)])       # 3/4, 3/4, 1/4 of a unit
        assert cf.truncate(x, dt).tolist() == [1.0, -1.0, 1.0] and cf.rne(x, dt).tolist() == [1.0 + 2.0 ** (1 - p), -1.0 - 2.0 ** (1 - p), 1.0]


# ------------------------------------------------------------------------------------------------ what the whole-clip bound lets through
def test_the_whole_clip_bound_lets_wrong_stand_ins_through():
    """test_gpu_refinenet.test_fused_cgru_scan_kernel_matches_per_step_path restated: max |diff| < 3e-2 and mean < 2e-3 against the
    per-frame stand-in of fake_kernels, bf16, its inputs (seed 11, B = 7, T = 5, h0).  Every wrong stand-in fails the judge; that
    bound lets two of them through: a filter element dropped at a border pixel (max 1.2e-2, mean 6.9e-4) and r * h formed from the
    unrounded r (1.2e-2, 6.5e-4).  It does catch the others here: the halo row of a neighbour (a whole row of taps: max 0.47), h_{t-2},
    x_{t+1}, and truncation (max 2.0e-2, but a mean of 2.5e-3)."""
    import fake_kernels
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    B, T = 7, 5
    inp = {'xs': (torch.randn((B, T, 5, 8, 64), generator=g) * 0.8).bfloat16(), 'h0': (torch.randn((B, 5, 8, 64), generator=g) * 0.5).bfloat16(),
           'w1': (torch.randn((128, 3, 3, 128), generator=g) * 0.04).bfloat16(), 'w2': (torch.randn((64, 3, 3, 128), generator=g) * 0.04).bfloat16()}
    inp['b1'], inp['b2'] = torch.randn((128,), generator=g) * 0.2, torch.randn((64,), generator=g) * 0.2
    want = fake_kernels.FakeKernels().cgru_scan_fwd(inp['xs'], inp['h0'], inp['w1'], inp['b1'], inp['w2'], inp['b2'])

    def old_check(got):
        worst = [((a.float() - b.float()).abs().max().item(), (a.float() - b.float()).abs().mean().item()) for a, b in zip(got, want)]
        return all(mx < 3e-2 and mean < 2e-3 for mx, mean in worst), worst

    assert old_check(run_fwd(inp, dt))[0] and judge_fwd(inp, dt, run_fwd(inp, dt)).ok
    let_through = []
    for fault in FWD_FAULTS:
        got = faulty_fwd(inp, dt, fault)
        passes, worst = old_check(got)
        print('%-10s old check %s (max %.1e, mean %.1e); judge %s' % (fault, 'passes' if passes else 'fails', max(w[0] for w in worst),
                                                                     max(w[1] for w in worst), 'passes' if judge_fwd(inp, dt, got).ok else 'fails'))
        assert not judge_fwd(inp, dt, got).ok
        if passes:
            let_through.append(fault)
    assert let_through == ['tap', 'raw_r'], let_through
