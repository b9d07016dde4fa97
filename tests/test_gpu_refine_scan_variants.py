"""GPU: RefineNet's clip-long conv-RNN scans for stacked cells (refine_net_rnn_num_cells > 1) and for the 32- / 128-wide
bottleneck (refine_net_num_features): the width-taking entry points eve_{cgru,crnn}_scan_{fwd,bwd}_c / eve_clstm_scan_fwd_c
(csrc/cell_scan_f32.hip) against the per-frame contract, the module against the reference-generated fixture
tests/golden/refinenet_variants.npz and against its own per-frame path, the 16-bit stacked scan against the rounding-faithful
oracle, and EVEStream over a stacked / wide bottleneck.  The CPU side: test_refine_scan_variants_host.py."""
import contextlib

import numpy as np
import pytest
import torch

import eve_amd
import refine_variants as rv
from eve_amd.kernels import default_kernels
from oracle import bf16_faithful as bf
from oracle import detweights
from test_gpu_stream import gpu_clip, make_model, maxdiff, run_chunks

pytestmark = pytest.mark.gpu
SCAN_SYMBOLS = ('cgru_scan', 'crnn_scan', 'clstm_scan')


@contextlib.contextmanager
def scan_symbols(k):
    """Records eve_last_kernel() right after every clip-scan forward the module issues."""
    seen, saved = [], {}
    for name in ('cgru_scan_fwd', 'crnn_scan_fwd', 'clstm_scan_fwd'):
        saved[name] = getattr(k, name)

        def wrapped(*a, _f=saved[name], **kw):
            out = _f(*a, **kw)
            seen.append(k.lib.eve_last_kernel().decode())
            return out
        setattr(k, name, wrapped)
    try:
        yield seen
    finally:
        for name in saved:
            delattr(k, name)


def kname(base, C):
    return base if C == 64 else '%s<%d>' % (base, C)


# ------------------------------------------------------------------------------------------------ 1. the entry points
@pytest.mark.parametrize('with_h0', [False, True], ids=['zero-state', 'h0'])
@pytest.mark.parametrize('B,T', [(1, 1), (1, 30), (5, 1), (5, 30), (32, 1), (32, 30)])
@pytest.mark.parametrize('C', [32, 128])
def test_width_taking_scan_entry_points_match_the_per_frame_contract(C, B, T, with_h0):
    """Float32 bounds of test_gpu_refinenet.test_float32_clip_scans_match_the_per_frame_contract (C = 64): 2e-5 forward, 3e-5
    backward (1e-4 over T = 30), relative to max(1, |reference|max).  A gate at C = 128 sums K = 2 304 products instead of
    1 152, so the reference itself is less exact there: the same ATen contract is evaluated in float32 and in float64 on these
    inputs and a tensor is allowed twice that deviation where it exceeds the C = 64 bound (printed per case).
    Measured on an MI355X at C = 128, B = 32, T = 30: forward <= 3.4e-6 (contract float32 vs float64: 5.4e-6), backward <= 6.9e-6
    (1.6e-6) -- the C = 64 bounds hold with margin and the float64 allowance never engaged.
    CGRU in bf16 at these widths runs the 16-bit-storage instantiation of the same kernel (checked last)."""
    hip = default_kernels()
    g = torch.Generator().manual_seed(100 * C + 10 * B + T)
    rn = lambda *shape, scale=1.0: torch.randn(shape, generator=g) * scale
    cu = lambda t: None if t is None else t.cuda()
    d = lambda t: None if t is None else t.double()
    s = 0.04 * (64.0 / C) ** 0.5                               # filter scale: the pre-activation variance of the C = 64 test
    xs, h0 = rn(B, T, 5, 8, C, scale=0.8), (rn(B, 5, 8, C, scale=0.5) if with_h0 else None)
    c0 = rn(B, 5, 8, C, scale=0.5) if with_h0 else None
    report = []

    def close(what, names, got, want, want64, tol):
        for name, a, b, b64 in zip(names, got, want, want64):
            if b is None:
                assert a is None, name
                continue
            a = a.float().cpu()
            assert tuple(a.shape) == tuple(b.shape), name
            err, ref_max = float((a - b).abs().max()), float(b.abs().max())
            ref_dev = float((b.double() - b64).abs().max())
            bound = max(tol * max(1.0, ref_max), 2.0 * ref_dev)
            report.append('%s.%s %.1e (f32-vs-f64 contract %.1e)' % (what, name, err, ref_dev))
            assert err <= bound, (what, name, err, bound, ref_dev)

    bwd_tol = 1e-4 if T > 8 else 3e-5
    # CGRU forward + backward (the backward on the float32 contract's own forward tensors)
    w1, w2 = rn(2 * C, 3, 3, 2 * C, scale=s), rn(C, 3, 3, 2 * C, scale=s)
    b1, b2 = rn(2 * C, scale=0.2), rn(C, scale=0.2)
    want = rv.contract_cgru_fwd(xs, h0, w1, b1, w2, b2)
    want64 = rv.contract_cgru_fwd(d(xs), d(h0), d(w1), d(b1), d(w2), d(b2))
    got = hip.cgru_scan_fwd(cu(xs), cu(h0), cu(w1), cu(b1), cu(w2), cu(b2))
    assert hip.lib.eve_last_kernel().decode() == kname('cgru_scan_f32_fwd_kernel', C)
    close('cgru_fwd', ('hs', 'hs_tm', 'ru', 'rh', 'og'), got, want, want64, 2e-5)
    dhs = rn(T, B, 5, 8, C)
    w1t, w2t = w1.permute(3, 1, 2, 0).contiguous(), w2.permute(3, 1, 2, 0).contiguous()
    hs_tm, ru, _, og = want[1:]
    want_b = rv.contract_cgru_bwd(dhs, ru, og, hs_tm, h0, w1t, w2t, with_h0)
    want_b64 = rv.contract_cgru_bwd(d(dhs), d(ru), d(og), d(hs_tm), d(h0), d(w1t), d(w2t), with_h0)
    got_b = hip.cgru_scan_bwd(cu(dhs), cu(ru), cu(og), cu(hs_tm), cu(h0), cu(w1t), cu(w2t), want_dh0=with_h0)
    assert hip.lib.eve_last_kernel().decode() == kname('cgru_scan_f32_bwd_kernel', C)
    close('cgru_bwd', ('dg1', 'dg2', 'dxs', 'dh0'), got_b, want_b, want_b64, bwd_tol)
    # CRNN forward + backward
    w, bias = rn(C, 3, 3, 2 * C, scale=s), rn(C, scale=0.2)
    want = rv.contract_crnn_fwd(xs, h0, w, bias)
    want64 = rv.contract_crnn_fwd(d(xs), d(h0), d(w), d(bias))
    got = hip.crnn_scan_fwd(cu(xs), cu(h0), cu(w), cu(bias))
    assert hip.lib.eve_last_kernel().decode() == kname('crnn_scan_f32_fwd_kernel', C)
    close('crnn_fwd', ('hs', 'hs_tm'), got, want, want64, 2e-5)
    wt = w.permute(3, 1, 2, 0).contiguous()
    want_b = rv.contract_crnn_bwd(dhs, want[1], wt, with_h0)
    want_b64 = rv.contract_crnn_bwd(d(dhs), d(want[1]), d(wt), with_h0)
    got_b = hip.crnn_scan_bwd(cu(dhs), cu(want[1]), cu(wt), want_dh0=with_h0)
    assert hip.lib.eve_last_kernel().decode() == kname('crnn_scan_f32_bwd_kernel', C)
    close('crnn_bwd', ('dpre', 'dxs', 'dh0'), got_b, want_b, want_b64, bwd_tol)
    # CLSTM forward (state (h, c); gate order in / forget / out / cell)
    w, bias = rn(4 * C, 3, 3, 2 * C, scale=s), rn(4 * C, scale=0.2)
    want = rv.contract_clstm_fwd(xs, h0, c0, w, bias)
    want64 = rv.contract_clstm_fwd(d(xs), d(h0), d(c0), d(w), d(bias))
    got = hip.clstm_scan_fwd(cu(xs), cu(h0), cu(c0), cu(w), cu(bias))
    assert hip.lib.eve_last_kernel().decode() == kname('clstm_scan_f32_fwd_kernel', C)
    close('clstm_fwd', ('hs', 'cs'), got, want, want64, 2e-5)
    print('C=%d B=%d T=%d: %s' % (C, B, T, ', '.join(report)))
    # CGRU in bf16 at this width (the 16-bit-storage instantiation), relative L2 <= 3e-3.  Forward: the scan's contract (float32
    # accumulation, the gates / r * h / state rounded to bf16; the per-frame stand-in of tests/fake_kernels.py also rounds the
    # convolution outputs, which the scans do not).  Backward: fake_kernels' restatement of the eve_cgru_scan_bwd contract.
    import fake_kernels
    fk = fake_kernels.FakeKernels()
    h16 = lambda t: None if t is None else t.bfloat16()
    v16 = lambda t: None if t is None else t.bfloat16().float()
    rel = lambda a, b: float((a.float().cpu().double() - b.float().double()).norm() / (b.float().double().norm() + 1e-30))
    want = [t.bfloat16() for t in rv.contract_cgru_fwd(v16(xs), v16(h0), v16(w1), b1, v16(w2), b2, rnd=v16)]
    got = hip.cgru_scan_fwd(cu(h16(xs)), cu(h16(h0)), cu(h16(w1)), cu(b1), cu(h16(w2)), cu(b2))
    assert hip.lib.eve_last_kernel().decode() == 'cgru_scan_f32_fwd_kernel<%d, eve::bf16_t>' % C
    for name, a, b in zip(('hs', 'hs_tm', 'ru', 'rh', 'og'), got, want):
        print('bf16 C=%d B=%d T=%d %s: relative L2 %.2e' % (C, B, T, name, rel(a, b)))
        assert a.dtype == torch.bfloat16 and tuple(a.shape) == tuple(b.shape) and rel(a, b) <= 3e-3, (name, rel(a, b))
    hs_tm, ru, _, og = want[1:]
    want_b = fk.cgru_scan_bwd(h16(dhs), ru, og, hs_tm, h16(h0), h16(w1t), h16(w2t), want_dh0=with_h0)
    got_b = hip.cgru_scan_bwd(cu(h16(dhs)), cu(ru), cu(og), cu(hs_tm), cu(h16(h0)), cu(h16(w1t)), cu(h16(w2t)), want_dh0=with_h0)
    assert hip.lib.eve_last_kernel().decode() == 'cgru_scan_f32_bwd_kernel<%d, eve::bf16_t>' % C
    for name, a, b in zip(('dg1', 'dg2', 'dxs', 'dh0'), got_b, want_b):
        if b is None:
            assert a is None, name
        else:
            print('bf16 C=%d B=%d T=%d %s: relative L2 %.2e' % (C, B, T, name, rel(a, b)))
            assert a.dtype == torch.bfloat16 and tuple(a.shape) == tuple(b.shape) and rel(a, b) <= 3e-3, (name, rel(a, b))


def test_an_unsupported_width_is_refused_without_a_launch():
    hip = default_kernels()
    C = 48
    z = lambda *s: torch.zeros(s, device='cuda')
    before = hip.lib.eve_last_kernel().decode()
    for call in (lambda: hip.cgru_scan_fwd(z(1, 1, 5, 8, C), None, z(2 * C, 3, 3, 2 * C), z(2 * C), z(C, 3, 3, 2 * C), z(C)),
                 lambda: hip.crnn_scan_fwd(z(1, 1, 5, 8, C), None, z(C, 3, 3, 2 * C), z(C)),
                 lambda: hip.clstm_scan_fwd(z(1, 1, 5, 8, C), None, None, z(4 * C, 3, 3, 2 * C), z(4 * C)),
                 lambda: hip.crnn_scan_bwd(z(1, 1, 5, 8, C), z(1, 1, 5, 8, C), z(2 * C, 3, 3, C))):
        with pytest.raises(RuntimeError, match='unsupported channel count'):
            call()
    assert hip.lib.eve_last_kernel().decode() == before
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the module, float32
@pytest.mark.parametrize('tag', sorted(rv.CASES))
def test_refinenet_variants_match_the_reference_fixture_on_the_scans(tag):
    """The five reference-generated cases through forward_sequence and through the per-step dict forward: heatmap_final and every
    cell's states at every frame <= 1e-4, gradient norms within 1e-2 (+ 3e-5 absolute: conv biases feeding an InstanceNorm have a
    zero gradient, what is computed there is rounding residue) -- the bounds test_gpu_refinenet holds the C = 64 fixture to.
    Every cell must have run as one clip-long scan of its width."""
    fx = rv.fixture()
    kind, width, cells = rv.CASES[tag]
    B, T = int(fx['B']), int(fx['T'])
    rb = rv.fixture_batch(fx)
    drb = {k: v.cuda() for k, v in rb.items()}
    net, cfg = rv.make_net(tag, weight_seed=int(fx['weight_seed']))
    net = net.cuda()
    with scan_symbols(default_kernels()) as seen:
        hf, states = net.forward_sequence(drb['heatmap_initial'], drb['screen_frame'])
    base = {'CGRU': 'cgru_scan_f32_fwd_kernel', 'CRNN': 'crnn_scan_f32_fwd_kernel', 'CLSTM': 'clstm_scan_f32_fwd_kernel'}[kind]
    assert seen == [kname(base, width)] * cells, seen
    want = fx[tag + '/heatmap_final']
    assert np.abs(hf.detach().cpu().numpy()[..., ::4, ::4] - want).max() < 1e-4
    assert want.std() > 1e-3
    assert len(states) == cells
    for (name, a), (_, b) in zip(rv.flat(states), rv.flat(rv.fixture_states(fx, tag))):
        assert tuple(a.shape) == tuple(b.shape) == (B, T, width, 5, 8), name
        assert np.abs(a.detach().cpu().numpy() - b).max() < 1e-4, name
    with torch.no_grad():
        hf_s, states_s = rv.per_step(net, drb['heatmap_initial'], drb['screen_frame'], cells)
    assert np.abs(hf_s.cpu().numpy()[..., ::4, ::4] - want).max() < 1e-4
    for (name, a), (_, b) in zip(rv.flat(states_s), rv.flat(rv.fixture_states(fx, tag))):
        assert np.abs(a.cpu().numpy() - b).max() < 1e-4, name
    from eve_amd import losses
    terms = losses.refinenet_loss_terms(hf, drb['heatmap_final_gt'], drb['validity'], cfg)
    np.testing.assert_allclose(float(terms['loss_ce_heatmap_final'].detach()), float(fx[tag + '/loss_ce']), rtol=2e-5)
    terms['full_loss'].backward()
    params, dead = dict(net.named_parameters()), 0
    for n, ref_norm in zip(fx[tag + '/grad_names'], fx[tag + '/grad_norms']):
        p = params[str(n)]
        if ref_norm < 0:
            assert p.grad is None, n
            dead += 1
        else:
            got = float(p.grad.double().norm())
            assert abs(got - ref_norm) <= 1e-2 * ref_norm + 3e-5, '%s: %.6g vs %.6g' % (n, got, ref_norm)
    assert dead == (2 * cells if kind == 'CLSTM' else 0)


@pytest.mark.parametrize('tag,dtype', [(t, torch.float32) for t in sorted(rv.CASES)] +
                         [(t, torch.bfloat16) for t in sorted(rv.CASES) if t.startswith('CGRU')],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_refinenet_variant_scans_train_like_the_per_frame_path(tag, dtype):
    """RefineNet forward + backward through the clip scans vs eve_dispatch_config.cgru_scan = 0 (the per-frame launches, what
    these configurations ran on before), bounds of test_gpu_refinenet.test_refinenet_clip_scans_train_like_the_per_frame_path.
    (CGRU in bf16 at C = 32 / 128: the 16-bit-storage instantiation of the float32 scan.)"""
    rb = detweights.refinenet_batch(3, 4, seed=3)
    kind, width, cells = rv.CASES[tag]
    outs = {}
    # (CGRU, bf16, C = 128) is left per frame by default (its scan measured slower): cgru_scan = 3 is the setting that scans it
    on = 3 if (dtype != torch.float32 and width == 128) else 1
    for mode in (on, 0):
        with default_kernels().dispatch_override(cgru_scan=mode):
            net, _ = rv.make_net(tag, dtype=dtype)
            net = net.cuda()
            with scan_symbols(default_kernels()) as seen:
                hf, states = net.forward_sequence(rb['heatmap_initial'].cuda(), rb['screen_frame'].cuda())
            (hf.float() * rb['heatmap_final_gt'].cuda()).sum().backward()
        assert len(seen) == (cells if mode != 0 else 0), (mode, seen)
        outs[mode] = (hf.detach().float().cpu(), [t.detach().float().cpu() for _, t in rv.flat(states)],
                      {n: p.grad.detach().float().cpu() for n, p in net.named_parameters() if p.grad is not None})
    a, b = outs[on], outs[0]
    f32 = dtype == torch.float32
    assert float((a[0] - b[0]).abs().max()) < (2e-5 if f32 else 0.05)
    assert len(a[1]) == len(b[1])
    for sa, sb in zip(a[1], b[1]):
        assert tuple(sa.shape) == tuple(sb.shape)
        assert float((sa - sb).abs().max()) < (2e-5 if f32 else 0.06)
    assert set(a[2]) == set(b[2])
    for n in b[2]:
        ga, gb = a[2][n], b[2][n]
        if ga.dim() < 2:
            continue          # biases feeding an InstanceNorm have an exactly-zero gradient: what is computed is rounding noise
        assert float((ga - gb).norm()) <= (2e-3 if f32 else 0.15) * float(gb.norm()) + 1e-4, n


# ------------------------------------------------------------------------------------------------ 3. bf16 vs the rounding-faithful oracle
def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / (want.norm() + 1e-30))


@pytest.mark.parametrize('tag', ['CGRU_c128_n1', 'CGRU_c64_n2'])
def test_bf16_rnn_stage_teacher_forced_matches_the_rounding_faithful_oracle(tag):
    """The `rnn` stage alone, teacher-forced through RefineNet._probe: the bottleneck gets a bf16-valued input and its output an
    output gradient, the oracle is oracle.bf16_faithful.cgru_step chained over frames and cells (rounding at the kernels'
    rounding points).  Output relative L2 <= 3e-3, input and parameter gradients <= 1e-2, as for the existing stage tests.
    (C = 64 x 2 cells runs the 16-bit MFMA scan twice; C = 128 the 16-bit-storage instantiation of the float32 scan.  The
    per-frame kernels, which round the gate convolutions' outputs to bf16 as well and are what bf16 at C = 128 runs by default,
    sit at 3.7e-3 from this oracle there.  Measured: forward 5.6e-4 / 7.6e-4, input gradient 4.3e-3 / 5.6e-3, worst parameter
    gradient 3.9e-3 / 6.8e-3 for the two cases.)"""
    kind, width, cells = rv.CASES[tag]
    B, T = 2, 5
    g = torch.Generator().manual_seed(7)
    x_in = (torch.randn(B * T, width, 5, 8, generator=g) * 0.8).bfloat16().float()
    dy = (torch.randn(B * T, width, 5, 8, generator=g) * 0.1).bfloat16().float()
    ref, _ = rv.make_oracle(tag)
    level = ref.network
    while hasattr(level, 'between_module'):
        level = level.between_module
    ocells = list(level.rnn_cells)
    assert len(ocells) == cells
    xo = x_in.clone().requires_grad_(True)
    with bf.rounding(True, torch.bfloat16):
        cur = xo.view(B, T, width, 5, 8)
        for cell in ocells:
            h, hs = torch.zeros_like(cur[:, 0]), []
            for t in range(T):
                h = bf.cgru_step(cell, cur[:, t], h)
                hs.append(h)
            cur = torch.stack(hs, dim=1)
        yo = cur.reshape(B * T, width, 5, 8)
        yo.backward(dy)
    net, _ = rv.make_net(tag, dtype=torch.bfloat16)
    net = net.cuda()
    rec, order = {}, []

    def probe(name, x):
        order.append(name)
        if name == 'rnn':
            assert order[-2] == 'enc4.1', order
            rec['out'] = x
        if name == 'enc4.1':
            rec['leaf'] = x_in.permute(0, 2, 3, 1).contiguous().to(x.dtype).cuda().requires_grad_(True)
            return rec['leaf']
        return x
    net._probe = probe
    rb = detweights.refinenet_batch(B, T, seed=2)
    # cgru_scan = 3: the setting under which every instantiated scan runs -- at C = 128 the 16-bit CGRU scan is off by default
    # because it measured slower (profiles/refine_scan_widths.md); this test is about that kernel
    with default_kernels().dispatch_override(cgru_scan=3), scan_symbols(default_kernels()) as seen:
        net.forward_sequence(rb['heatmap_initial'].cuda(), rb['screen_frame'].cuda())
    assert len(seen) == cells, seen
    out = rec['out']
    out.backward(dy.permute(0, 2, 3, 1).contiguous().to(out.dtype).cuda())
    e = rel_l2(out.float().cpu().permute(0, 3, 1, 2), yo)
    assert e <= 3e-3, 'rnn stage forward: relative L2 %.3e' % e
    eb = rel_l2(rec['leaf'].grad.float().cpu().permute(0, 3, 1, 2), xo.grad)
    assert eb <= 1e-2, 'gradient entering the rnn stage: relative L2 %.3e' % eb
    params, rparams, worst = dict(net.named_parameters()), dict(ref.named_parameters()), 0.0
    names = [n for n in params if '.rnn_cells.' in n]
    assert len(names) == 4 * cells
    for n in names:
        ep = rel_l2(params[n].grad, rparams[n].grad)
        worst = max(worst, ep)
        assert ep <= 1e-2, '%s: gradient relative L2 %.3e' % (n, ep)
    print('%s rnn stage: forward %.2e, input gradient %.2e, worst parameter gradient %.2e' % (tag, e, eb, worst))


# ------------------------------------------------------------------------------------------------ 4. streaming
@pytest.mark.parametrize('over', [dict(refine_net_rnn_type='CGRU', refine_net_rnn_num_cells=2),
                                  dict(refine_net_rnn_type='CGRU', refine_net_num_features=128)], ids=['cgru-2-cells', 'cgru-128-wide'])
def test_stream_over_a_stacked_or_wide_bottleneck_matches_the_whole_clip(over):
    """A 30-frame clip of two streams in chunks of 7 + 1 + 22 frames through EVEStream with graph mode on equals one eval pass
    (bounds of test_gpu_stream.test_stream_float32_matches_the_whole_clip), and get_state / set_state round-trip every cell."""
    model, _ = make_model('refine_net.json', **over)
    b, d, full = gpu_clip(2, 30)
    with torch.no_grad():
        whole = model(dict(full))
    stream = eve_amd.EVEStream(model, 2)
    assert stream.use_graph
    got = run_chunks(stream, d, [7, 1, 22])
    for k, v in got.items():
        if k in whole:
            e = maxdiff(v, whole[k])
            amp = 5.0 if k.endswith('_final') else 1.0
            assert e <= amp * (1e-2 if 'px' in k else (1e-3 if 'cm' in k else 1e-5)), (k, e)
    st = stream.get_state()
    C, n = over.get('refine_net_num_features', 64), over.get('refine_net_rnn_num_cells', 1)
    for i in range(n):
        assert tuple(st['refinenet_rnn_states_%d' % i].shape) == (2, C, 5, 8)
    assert 'refinenet_rnn_states_%d' % n not in st
    other = eve_amd.EVEStream(model, 2)
    other.set_state(st)
    for k, v in other.get_state().items():
        assert torch.equal(v, st[k]), k
    nxt = {k: v[:, :3].contiguous() for k, v in d.items()}
    oa, ob = stream.step(nxt), other.step(nxt)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
