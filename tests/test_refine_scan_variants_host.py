"""CPU: stacked conv-RNN cells and the 32- / 128-wide bottleneck of RefineNet (refine_net_rnn_num_cells, refine_net_num_features)
on the clip-scan branch of RefineNet.forward_sequence, with the ATen stand-ins of tests/fake_kernels.py, against the oracle and
the reference-generated fixture tests/golden/refinenet_variants.npz.  The HIP kernels: test_gpu_refine_scan_variants.py."""
import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import kernels
from eve_amd.refine_net import RefineNet
import refine_variants as rv
from oracle import sequence
from test_stream_host import StreamFakes, chunk_of, clip, make_model, run_chunks, tol


class CountingFakes(StreamFakes):
    """StreamFakes that records which clip scans ran."""

    def cgru_scan_fwd(self, *a, **k):
        self.calls.append('cgru_scan_fwd')
        return super().cgru_scan_fwd(*a, **k)

    def crnn_scan_fwd(self, *a, **k):
        self.calls.append('crnn_scan_fwd')
        return super().crnn_scan_fwd(*a, **k)

    def clstm_scan_fwd(self, *a, **k):
        self.calls.append('clstm_scan_fwd')
        return super().clstm_scan_fwd(*a, **k)


@pytest.fixture()
def fake():
    k = CountingFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


@pytest.mark.parametrize('tag', sorted(rv.CASES))
def test_oracle_reproduces_the_variant_fixture(tag):
    """Bounds of test_oracle_golden.test_refinenet_matches_reference (refinenet.npz): 3e-6 absolute on heat-map and states, 3e-6
    relative on the loss, gradient norms rtol 5e-4 + 2e-5."""
    fx = rv.fixture()
    kind, width, cells = rv.CASES[tag]
    rb = rv.fixture_batch(fx)
    net, cfg = rv.make_oracle(tag, int(fx['weight_seed']))
    hf, states = rv.per_step(net, rb['heatmap_initial'], rb['screen_frame'], cells)
    want = fx[tag + '/heatmap_final']
    np.testing.assert_allclose(hf.detach().numpy()[..., ::4, ::4], want, atol=3e-6)
    assert want.std() > 1e-3
    for (name, got), (_, ref) in zip(rv.flat(states), rv.flat(rv.fixture_states(fx, tag))):
        assert tuple(got.shape) == tuple(ref.shape) == (int(fx['B']), int(fx['T']), width, 5, 8), name
        np.testing.assert_allclose(got.detach().numpy(), ref, atol=3e-6, err_msg=name)
    terms = sequence.refinenet_losses(hf, rb['heatmap_final_gt'], rb['validity'], cfg)
    np.testing.assert_allclose(float(terms['loss_ce_heatmap_final'].detach()), float(fx[tag + '/loss_ce']), rtol=3e-6)
    terms['full_loss'].backward()
    params, dead = dict(net.named_parameters()), 0
    assert [str(n) for n in fx[tag + '/grad_names']] == list(params)
    for n, ref_norm in zip(fx[tag + '/grad_names'], fx[tag + '/grad_norms']):
        p = params[str(n)]
        if ref_norm < 0:                     # CLSTM dead-output quirk (refine_net.py:168-174): EVERY cell of the stack
            assert p.grad is None, n
            dead += 1
        else:
            np.testing.assert_allclose(float(p.grad.double().norm()), ref_norm, rtol=5e-4, atol=2e-5, err_msg=str(n))
    assert dead == (2 * cells if kind == 'CLSTM' else 0)


def test_scan_rule():
    """Which (cell, width, count, format) combinations RefineNet._use_scan sends through the clip scans."""
    from eve_amd.refine_net import CGRUCell, CLSTMCell, CRNNCell
    kernels.set_default_kernels(CountingFakes())
    try:
        for n in (1, 2, 3):
            for C in (32, 64, 128):
                for dt in (torch.float32, torch.bfloat16, torch.float16):
                    # 16-bit CGRU / CLSTM at 128 measured slower than the per-frame path (profiles/refine_scan_widths.md)
                    off = C == 128 and dt != torch.float32
                    assert RefineNet._use_scan([CRNNCell(C, C)] * n, (5, 8, C), dt)
                    assert RefineNet._use_scan([CLSTMCell(C, C)] * n, (5, 8, C), dt) == (not off)
                    assert RefineNet._use_scan([CGRUCell(C, C)] * n, (5, 8, C), dt) == (not off)
        assert not RefineNet._use_scan([], (5, 8, 64), torch.float32)
        assert not RefineNet._use_scan([CGRUCell(48, 48)], (5, 8, 48), torch.float32)
        assert not RefineNet._use_scan([CGRUCell(64, 64)], (9, 16, 64), torch.float32)
    finally:
        kernels.set_default_kernels(None)


@pytest.mark.parametrize('tag', sorted(rv.CASES))
def test_forward_sequence_scans_every_cell_and_matches_per_step_oracle_and_fixture(fake, tag):
    fx = rv.fixture()
    kind, width, cells = rv.CASES[tag]
    rb = rv.fixture_batch(fx)
    net, cfg = rv.make_net(tag, weight_seed=int(fx['weight_seed']))
    ref, ocfg = rv.make_oracle(tag, int(fx['weight_seed']))
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    hf, states = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'])
    scan = {'CGRU': 'cgru_scan_fwd', 'CRNN': 'crnn_scan_fwd', 'CLSTM': 'clstm_scan_fwd'}[kind]
    assert fake.calls.count(scan) == cells, fake.calls          # the scan branch: one clip-long launch per cell
    assert len(states) == cells
    # the per-step dict contract on the same kernels
    with torch.no_grad():
        hf_s, states_s = rv.per_step(net, rb['heatmap_initial'], rb['screen_frame'], cells)
    assert float((hf.detach() - hf_s).abs().max()) < 1e-5
    for (name, a), (_, b) in zip(rv.flat(states), rv.flat(states_s)):
        assert tuple(a.shape) == tuple(b.shape) == (int(fx['B']), int(fx['T']), width, 5, 8), name
        assert float((a.detach() - b).abs().max()) < 1e-5, name
    # the oracle and the reference's own numbers
    with torch.no_grad():
        hf_o, states_o = rv.per_step(ref, rb['heatmap_initial'], rb['screen_frame'], cells)
    assert float((hf.detach() - hf_o).abs().max()) < 1e-4
    assert np.abs(hf.detach().numpy()[..., ::4, ::4] - fx[tag + '/heatmap_final']).max() < 1e-4
    for (name, a), (_, b), (_, c) in zip(rv.flat(states), rv.flat(states_o), rv.flat(rv.fixture_states(fx, tag))):
        assert float((a.detach() - b).abs().max()) < 1e-4, name
        assert np.abs(a.detach().numpy() - c).max() < 1e-4, name
    # gradients through the chained scans: the fixture's norms (no gradient reaches any CLSTM weight)
    sequence.refinenet_losses(hf, rb['heatmap_final_gt'], rb['validity'], ocfg)['full_loss'].backward()
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


@pytest.mark.parametrize('over', [dict(refine_net_rnn_type='CGRU', refine_net_rnn_num_cells=2),
                                  dict(refine_net_rnn_type='CLSTM', refine_net_rnn_num_cells=2, refine_net_num_features=32)],
                         ids=['cgru-2-cells', 'clstm-2-cells-32-wide'])
def test_stream_of_a_stacked_model_chunked_equals_whole_clip(fake, over):
    """The contract of test_stream_host.py for a two-cell bottleneck: chunks through EVEStream equal one eval pass of the clip;
    every cell's carried state is its own last frame; get_state / set_state round-trip both cells."""
    model, _ = make_model(over)
    batch = clip(1, 12, seed=9)
    stream = eve_amd.EVEStream(model, 1, use_graph=False)
    got = run_chunks(stream, batch, [5, 1, 6])
    with torch.no_grad():
        whole = model(dict(batch))
    for k in got:
        if k in whole:
            assert float((got[k] - whole[k]).abs().max()) < tol(k), k
    st = stream.get_state()
    C = over.get('refine_net_num_features', 64)
    for i in range(2):
        v = st['refinenet_rnn_states_%d' % i]
        for t in v if isinstance(v, tuple) else (v,):
            assert tuple(t.shape) == (1, C, 5, 8) and float(t.abs().max()) > 0
    assert not torch.equal(*[(v[0] if isinstance(v, tuple) else v) for v in (st['refinenet_rnn_states_0'], st['refinenet_rnn_states_1'])])
    other = eve_amd.EVEStream(model, 1, use_graph=False)
    other.set_state(st)
    for k, v in other.get_state().items():
        for x, y in zip(v if isinstance(v, tuple) else (v,), st[k] if isinstance(st[k], tuple) else (st[k],)):
            assert torch.equal(x, y), k
    nxt = clip(1, 3, seed=10)
    oa, ob = stream.step(chunk_of(nxt, 0, 3)), other.step(chunk_of(nxt, 0, 3))
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
