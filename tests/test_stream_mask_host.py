"""CPU: masked EVEStream steps (step(chunk, eye_mask=..., skip_invalid_pose=...)) on the torch-CPU stand-in kernels -- argument
checks, the valid / eye_valid outputs and the contract: every eye sequence consumes exactly its usable frames, every stream's
RefineNet exactly its valid frames, and the binocular quantities of a frame come from its usable eyes alone.  The stand-in of
tests/test_stream_ragged_host.py is extended here by restatements of the two masked entry points (eve_stream_mask_plan,
eve_stream_permute_rows); tests/test_gpu_stream_mask.py checks the HIP kernels and the graph mode."""
import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import kernels, ops
from test_stream_host import chunk_of, clip, tol
from test_stream_ragged_host import CONFIGS, RaggedFakes, flat_state, make_model, padded_chunk

B_CLIP, T_CLIP, TC = 3, 10, 4
LAST = T_CLIP - 2 * TC                                   # frames of the partial last step: lengths = [LAST] * B there
bits = lambda s: [c == '1' for c in s]
# per stream (left, right): a control; both / left-only / right-only / none with a hole of two invalid frames inside the second
# chunk; a whole first chunk with nothing usable and an eye with two usable frames
MASKS = [('1111111111', '1111111111'), ('1101100111', '1011100101'), ('0000111100', '0000011000')]
MASK = torch.tensor([[bits(l), bits(r)] for l, r in MASKS]).permute(0, 2, 1).contiguous()          # bool [B, T, 2]
assert int(MASK.any(-1).sum()) == 22


def numpy_plan(B, T, mask=None, pose_valid=None, lengths=None):
    """include/eve_hip.h eve_stream_mask_plan restated: -> count [3B], perm, inv [3B, T] int32, eye_valid [B, T, 2], valid [B, T] uint8."""
    ok = np.ones((B, T, 2), dtype=bool)
    for m in (mask, pose_valid):
        ok &= True if m is None else np.asarray(m).reshape(B, T, 2) != 0
    if lengths is not None:
        n = np.clip(np.asarray(lengths, dtype=np.int64)[:2 * B], 0, T).reshape(2, B)
        ok &= np.arange(T)[None, :, None] < n.T[:, None, :]
    use = np.concatenate([ok[:, :, 0], ok[:, :, 1], ok.any(-1)], axis=0)                       # eye rows (left, right), frame rows
    perm = np.argsort(~use, axis=1, kind='stable').astype(np.int32)                            # usable ascending, then the others
    inv = np.argsort(perm, axis=1, kind='stable').astype(np.int32)
    return use.sum(1).astype(np.int32), perm, inv, ok.astype(np.uint8), ok.any(-1).astype(np.uint8)


class MaskFakes(RaggedFakes):
    """RaggedFakes plus include/eve_hip.h eve_stream_mask_plan and eve_stream_permute_rows."""

    def stream_mask_plan(self, B, T, mask=None, pose_valid=None, lengths=None, device=None):
        self.calls.append('stream_mask_plan')
        arr = lambda t: None if t is None else t.contiguous().view(torch.uint8).numpy() if t.dtype == torch.bool else t.numpy()
        names = ('count', 'perm', 'inv', 'eye_valid', 'valid')
        return dict(zip(names, (torch.from_numpy(a) for a in numpy_plan(B, T, arr(mask), arr(pose_valid), arr(lengths)))))

    def stream_permute_rows(self, src, index):
        self.calls.append('stream_permute_rows')
        idx = index.long().clamp(0, src.shape[1] - 1)
        return torch.stack([src[s][idx[s]] for s in range(src.shape[0])], dim=0).contiguous()


@pytest.fixture()
def fake():
    k = MaskFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


# ------------------------------------------------------------------------------------------------ the reference
def masked_reference(model, batch, mask):
    """The contract, frame by frame, from the modules' public calls: EyeNet.forward_sequence on one frame with initial_states, a
    sequence's new state kept only where its eye is usable; the fusion rule written out; RefineNet.forward_sequence on one frame
    with initial_states, the new state kept only where the frame is valid.  batch: [B, T, ...] inputs; mask: bool [B, T, 2].
    -> (outputs [B, T, ...] -- meaningful at valid frames / usable eyes only --, states in EVEStream.get_state()'s layout)."""
    cfg, k = model.config, kernels.default_kernels()
    B, T = mask.shape[:2]
    screen = tuple(cfg.actual_screen_size)
    w, h = cfg.gaze_heatmap_size
    sides = ('left', 'right')
    keep = lambda m, new, old: torch.where(m.view((B,) + (1,) * (new.dim() - 1)), new, old)
    keep_st = lambda m, new, old: tuple(keep(m, n, o) for n, o in zip(new, old)) if isinstance(new, tuple) else keep(m, new, old)
    mean2 = lambda a, b: torch.stack([a, b], dim=-1).mean(dim=-1)
    eye_st, ref_st, outs = None, None, []
    with torch.no_grad():
        for t in range(T):
            fr = {k_: v[:, t:t + 1].contiguous() for k_, v in batch.items()}
            l, r = mask[:, t, 0], mask[:, t, 1]
            e = model.eye_net.forward_sequence(fr, initial_states=eye_st)
            ncell = len([k_ for k_ in e if k_.startswith('left_eye_rnn_states_')])
            last = lambda st: tuple(s_[:, 0] for s_ in st) if isinstance(st, tuple) else st[:, 0]
            new = {s_: [last(e['%s_eye_rnn_states_%d' % (s_, i)]) for i in range(ncell)] for s_ in sides}
            if eye_st is None:
                zero = lambda st: tuple(torch.zeros_like(s_) for s_ in st) if isinstance(st, tuple) else torch.zeros_like(st)
                eye_st = {s_: [zero(st) for st in new[s_]] for s_ in sides}
            eye_st = {s_: [keep_st(mask[:, t, si], n, o) for n, o in zip(new[s_], eye_st[s_])] for si, s_ in enumerate(sides)}
            o = {k_: e[k_][:, 0] for k_ in ('left_g_initial', 'right_g_initial', 'left_pupil_size', 'right_pupil_size')}
            # the fusion rule: both eyes usable -> the mean; one -> that eye's own; the rotation is left_R where the left eye is usable
            pog = {}
            for s_ in sides:
                _, mm, px = ops.GazeToPoGFn.apply(o[s_ + '_g_initial'], fr[s_ + '_o'][:, 0].float(), fr[s_ + '_R'][:, 0].float(),
                                                  fr['inv_camera_transformation'][:, 0].float(), fr['pixels_per_millimeter'][:, 0].float(),
                                                  screen, None, None)
                pog[s_] = {'px': px, 'cm': 0.1 * mm, 'o': fr[s_ + '_o'][:, 0]}
            fuse = lambda a, b: keep(l & r, mean2(a, b), keep(l, a, b))
            origin = fuse(pog['left']['o'], pog['right']['o'])
            rot = keep(l, fr['left_R'][:, 0], fr['right_R'][:, 0])
            cam = fr['camera_transformation'][:, 0].float()
            for unit in ('px', 'cm'):
                o['PoG_%s_initial' % unit] = fuse(pog['left'][unit], pog['right'][unit])
            o['g_initial'] = k.combined_gaze(origin.float(), 10.0 * o['PoG_cm_initial'], rot.float(), cam)
            hm = ops.MakeHeatmapsFn.apply(o['PoG_px_initial'], cfg.gaze_heatmap_sigma_initial, (h, w), screen).view(B, 1, 1, h, w)
            hf, st = model.refine_net.forward_sequence(hm, fr.get('screen_frame'), initial_states=ref_st)
            new = [last(s_) for s_ in st]
            if ref_st is None:
                ref_st = [zero(s_) for s_ in new]
            ref_st = [keep_st(l | r, n, o_) for n, o_ in zip(new, ref_st)]
            px = ops.SoftArgmaxFn.apply(hf.reshape(B, 1, hf.shape[-2], hf.shape[-1]).float(), screen)
            o['PoG_px_final'] = px
            o['PoG_cm_final'] = px * (0.1 * fr['millimeters_per_pixel'][:, 0])
            o['g_final'] = k.combined_gaze(origin.float(), 10.0 * o['PoG_cm_final'], rot.float(), cam)
            outs.append(o)
    state = {'%s_eye_rnn_states_%d' % (s_, i): st for s_ in sides for i, st in enumerate(eye_st[s_])}
    state.update({'refinenet_rnn_states_%d' % i: st for i, st in enumerate(ref_st)})
    return {k_: torch.stack([o[k_] for o in outs], dim=1) for k_ in outs[0]}, state


_REFERENCE = {}


def reference_for(name):
    """masked_reference of the test clip under MASK for one entry of CONFIGS, computed once and shared (never modified)."""
    if name not in _REFERENCE:
        over, _ = CONFIGS[name]
        _REFERENCE[name] = masked_reference(make_model(over), chunk_of(clip(B_CLIP, T_CLIP), 0, T_CLIP), MASK)
    return _REFERENCE[name]


def step_masks(mask=MASK):
    """Per step of TC frames: (the first frame, the [B, TC, 2] mask -- ones where the clip has no frame: lengths cut those --, lengths)."""
    steps = []
    for t0 in range(0, T_CLIP, TC):
        m = torch.ones((mask.shape[0], TC, 2), dtype=torch.bool)
        n = min(TC, T_CLIP - t0)
        m[:, :n] = mask[:, t0:t0 + n]
        steps.append((t0, m, None if n == TC else [n] * mask.shape[0]))
    return steps


def run_masked(stream, batch, mask=MASK, junk=None, as_form=lambda m: m, pad=padded_chunk):
    """Step the clip in chunks of TC frames under the mask (the last step padded with random finite junk and cut by lengths);
    junk: None, or callable(chunk, usable [B, TC, 2] bool, seed) -> chunk applied to every step's chunk; as_form: the form the
    step's bool [B, TC, 2] CPU mask is handed over in; pad: padded_chunk or its GPU twin.  -> ([B, T, ...] outputs including
    valid / eye_valid, the stream's state)."""
    parts = []
    for i, (t0, m, lengths) in enumerate(step_masks(mask)):
        ch = pad(batch, [t0] * mask.shape[0], TC, 11 + i)
        n = TC if lengths is None else lengths[0]
        if junk is not None:
            usable = m.clone()
            usable[:, n:] = False
            ch = junk(ch, usable, 100 + i)
        out = stream.step(ch, lengths=lengths, eye_mask=as_form(m))
        parts.append({k_: v[:, :n].clone() for k_, v in out.items()})
    return {k_: torch.cat([p[k_] for p in parts], dim=1) for k_ in parts[0]}, stream.get_state()


PER_EYE = {'left_g_initial': 0, 'left_pupil_size': 0, 'right_g_initial': 1, 'right_pupil_size': 1}


def where_defined(key, mask=MASK):
    """bool [B, T]: the entries of an output the contract defines -- usable eyes for a per-eye key, valid frames otherwise."""
    return mask[:, :, PER_EYE[key]] if key in PER_EYE else mask.any(-1)


def junk_unusable(chunk, usable, seed):
    """The chunk with seeded random finite values in everything a masked-out eye supplied (patch, h, o, R) and in every input of
    a frame without a usable eye."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda v: (torch.randint(0, 256, v.shape, generator=g, dtype=torch.uint8) if v.dtype == torch.uint8 else
                     3.0 * torch.randn(v.shape, generator=g).to(v.dtype))
    out = {k_: v.clone() for k_, v in chunk.items()}
    for k_, v in out.items():
        side = {'left': 0, 'right': 1}.get(k_.split('_')[0])
        gone = ~usable[:, :, side] if side is not None and k_.split('_', 1)[1] in ('eye_patch', 'h', 'o', 'R') else ~usable.any(-1)
        v[gone.to(v.device)] = rnd(v)[gone].to(v.device)
    return out


# ------------------------------------------------------------------------------------------------ arguments and the output keys
def test_mask_arguments_are_validated(fake):
    model = make_model(dict(refine_net_rnn_type='CGRU'))
    s = eve_amd.EVEStream(model, 2, use_graph=False)
    ch = chunk_of(clip(2, 3, seed=5), 0, 3)
    ones = np.ones((2, 3, 2), dtype=bool)
    for bad in (ones[:1], ones[:, :2], ones[:, :, :1], ones.reshape(2, 6), ones.astype(np.float32), torch.ones((2, 3, 2)),
                [[[1.0, 1.0]] * 3] * 2, [1, 0]):
        with pytest.raises(ValueError):
            s.step(ch, eye_mask=bad)
    with pytest.raises(ValueError):
        s.step(ch, skip_invalid_pose=True)                         # no eye_pose in the chunk: no pose_valid to fold in
    with pytest.raises(ValueError):
        s.step(ch, eye_mask=ones, lengths=[1, 4])                  # lengths are still checked
    assert not fake.calls                                         # a refused step has launched nothing
    for good in (ones, ones.astype(np.uint8), torch.from_numpy(ones), ones.astype(np.int64).tolist(), ones.tolist()):
        s.step(ch, eye_mask=good)
    assert 'stream_mask_plan' in fake.calls and 'stream_permute_rows' in fake.calls


def test_valid_and_eye_valid_only_on_masked_steps(fake):
    model = make_model(dict(refine_net_rnn_type='CGRU'))
    s = eve_amd.EVEStream(model, 3, use_graph=False)
    ch = chunk_of(clip(3, 4, seed=5), 0, 4)
    plain = s.step(ch)
    assert 'valid' not in plain and 'eye_valid' not in plain
    assert 'eye_valid' not in s.step(ch, lengths=[4, 0, 2])
    m = MASK[:, 4:8]
    out = s.step(ch, eye_mask=m, lengths=[4, 3, 1])
    want = m.clone()
    want[1, 3:] = False
    want[2, 1:] = False
    assert out['eye_valid'].dtype == torch.bool and tuple(out['eye_valid'].shape) == (3, 4, 2)
    assert out['valid'].dtype == torch.bool and tuple(out['valid'].shape) == (3, 4)
    assert torch.equal(out['eye_valid'], want) and torch.equal(out['valid'], want.any(-1))
    assert set(out) == set(plain) | {'valid', 'eye_valid'}
    for k_, v in plain.items():
        assert out[k_].shape == v.shape, k_
    assert 'valid' not in s.step(ch)
    assert fake.calls.count('stream_mask_plan') == 1              # one plan launch per masked step, none on the others


# ------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_masked_stream_matches_the_frame_by_frame_reference(fake, name):
    """Three streams, one 10-frame clip, steps of 4 frames under MASK (the last step partial: random junk in its last two
    frames, lengths = [2, 2, 2], so mask and lengths combine): every one of the 22 valid frames, and the per-eye keys at every
    usable eye, equal masked_reference within test_stream_host.tol; the carried states afterwards equal the reference's within
    the ragged host test's bounds for states."""
    over, fused = CONFIGS[name]
    want, want_state = reference_for(name)
    model = make_model(over, fused)
    got, state = run_masked(eve_amd.EVEStream(model, B_CLIP, use_graph=False), chunk_of(clip(B_CLIP, T_CLIP), 0, T_CLIP))
    assert ('eye_tail_stream_fwd_len' in fake.calls) == fused and 'eye_tail_stream_fwd' not in fake.calls
    assert torch.equal(got.pop('eye_valid'), MASK) and torch.equal(got.pop('valid'), MASK.any(-1))
    assert set(got) == set(want)
    compared = 0
    for k_, v in got.items():
        at = where_defined(k_)
        compared += int(at.sum()) if k_ == 'g_final' else 0
        err = float((v[at] - want[k_][at]).abs().max())
        assert torch.isfinite(v[at]).all() and err < tol(k_), (k_, err)
    assert compared == 22
    for (k_, i, a), (k2, _, b) in zip(flat_state(state), flat_state(want_state)):
        assert k_ == k2
        assert float((a - b).abs().max()) < tol('g_final' if k_.startswith('refinenet') else 'g_initial'), (k_, i)


@pytest.mark.parametrize('name', ['gru-cgru', 'gru-cgru-fused-tail', 'lstm-crnn', 'clstm-live'])
def test_masked_out_inputs_reach_no_valid_output(fake, name):
    """The same run with every masked-out eye's patch, h, o and R replaced by seeded random finite values, and every input of a
    frame without a usable eye randomised: the valid outputs and the carried states do not change by a bit."""
    over, fused = CONFIGS[name]
    model = make_model(over, fused)
    batch = chunk_of(clip(B_CLIP, T_CLIP), 0, T_CLIP)
    clean, clean_state = run_masked(eve_amd.EVEStream(model, B_CLIP, use_graph=False), batch)
    dirty, dirty_state = run_masked(eve_amd.EVEStream(model, B_CLIP, use_graph=False), batch, junk=junk_unusable)
    for k_, v in clean.items():
        at = where_defined(k_) if k_ not in ('valid', 'eye_valid') else torch.ones(MASK.shape[:2], dtype=torch.bool)
        assert torch.equal(v[at], dirty[k_][at]), k_
    for (k_, i, a), (_, _, b) in zip(flat_state(clean_state), flat_state(dirty_state)):
        assert torch.equal(a, b), (k_, i)


@pytest.mark.parametrize('name', ['gru-cgru', 'gru-cgru-fused-tail', 'clstm'])
def test_all_ones_mask_gives_the_unmasked_bits(fake, name):
    over, fused = CONFIGS[name]
    model = make_model(over, fused)
    batch = clip(B_CLIP, 2 * TC)
    a, b = eve_amd.EVEStream(model, B_CLIP, use_graph=False), eve_amd.EVEStream(model, B_CLIP, use_graph=False)
    for t0 in (0, TC):
        ch = chunk_of(batch, t0, t0 + TC)
        plain, masked = a.step(ch), b.step(ch, eye_mask=np.ones((B_CLIP, TC, 2), dtype=bool))
        assert masked.pop('valid').all() and masked.pop('eye_valid').all()
        for k_ in plain:
            assert torch.equal(plain[k_], masked[k_]), (t0, k_)
    for (k_, i, x), (_, _, y) in zip(flat_state(a.get_state()), flat_state(b.get_state())):
        assert torch.equal(x, y), (k_, i)


def test_frame_level_mask_equals_the_compacted_ragged_step(fake):
    """Both columns equal: the valid outputs equal those of the chunk compacted on the host (every stream's valid frames moved
    to the front) and stepped with lengths = the valid counts through the ragged interface."""
    model = make_model(*CONFIGS['gru-cgru'])
    batch = clip(B_CLIP, 2 * TC)
    frames = torch.tensor([[bits('1011'), bits('0110'), bits('0000')], [bits('0101'), bits('1111'), bits('0010')]])     # [step][B][TC]
    masked, ragged = eve_amd.EVEStream(model, B_CLIP, use_graph=False), eve_amd.EVEStream(model, B_CLIP, use_graph=False)
    for i, fm in enumerate(frames):
        ch = chunk_of(batch, i * TC, (i + 1) * TC)
        order = torch.argsort((~fm).to(torch.int8), dim=1, stable=True)
        packed = {k_: torch.stack([v[b][order[b]] for b in range(B_CLIP)], dim=0).contiguous() for k_, v in ch.items()}
        got = masked.step(ch, eye_mask=torch.stack([fm, fm], dim=-1))
        want = ragged.step(packed, lengths=fm.sum(1).tolist())
        assert torch.equal(got['valid'], fm)
        for k_ in want:
            if k_ != 'valid':
                for b in range(B_CLIP):
                    n = int(fm[b].sum())
                    if n:
                        assert float((got[k_][b][fm[b]] - want[k_][b, :n]).abs().max()) < tol(k_), (i, k_, b)
    for (k_, j, x), (_, _, y) in zip(flat_state(masked.get_state()), flat_state(ragged.get_state())):
        assert float((x - y).abs().max()) < tol('g_final' if k_.startswith('refinenet') else 'g_initial'), (k_, j)


@pytest.mark.parametrize('fused', [False, True], ids=['layers', 'fused-tail'])
def test_reset_reaches_a_stream_without_usable_frames(fake, fused):
    model = make_model(dict(refine_net_rnn_type='CLSTM'), fused)
    batch = clip(2, 6, seed=7)
    s = eve_amd.EVEStream(model, 2, use_graph=False)
    s.step(chunk_of(batch, 0, 3))
    before = flat_state(s.get_state())
    s.reset([1])
    s.step(chunk_of(batch, 3, 6), eye_mask=np.zeros((2, 3, 2), dtype=bool))
    for (k_, i, a), (_, _, b) in zip(flat_state(s.get_state()), before):
        assert torch.equal(a[0], b[0]), k_                        # stream 0: nothing usable, no reset -- untouched, bit for bit
        assert not a[1].any() and b[1].any(), k_                  # stream 1: zero state
    # one eye without usable frames keeps its EyeNet state while the other eye and RefineNet move on
    m = np.zeros((2, 3, 2), dtype=bool)
    m[0, :, 1] = True
    mid = flat_state(s.get_state())
    s.step(chunk_of(batch, 3, 6), eye_mask=m)
    for (k_, i, a), (_, _, b) in zip(flat_state(s.get_state()), mid):
        assert torch.equal(a[0], b[0]) == k_.startswith('left'), k_
        assert torch.equal(a[1], b[1]), k_
