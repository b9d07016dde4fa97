"""CPU: ragged EVEStream steps (step(chunk, lengths=...)) on the torch-CPU stand-in kernels -- argument checks, the `valid` mask,
the contract (a clip consumed at a different pace per stream equals the whole clip) and that a step without lengths issues the
kernel calls it issued before ragged steps existed.  The stand-in of tests/test_stream_host.py is extended here by restatements
of the two ragged entry points (eve_stream_state_rows_at, eve_eye_tail_stream_fwd_len); tests/test_gpu_stream_ragged.py checks
the HIP kernels and the graph mode."""
import json
import os

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import kernels
from oracle import detweights
from test_stream_host import StreamFakes, chunk_of, clip, tol

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CALLS = os.path.join(REPO, 'tests', 'golden', 'stream_uniform_calls.json')

# the configurations the ragged contract is stated for: (config overrides, EyeNet.stream_fused_tail)
CONFIGS = {
    'gru-cgru': (dict(refine_net_rnn_type='CGRU'), False),
    'gru-cgru-fused-tail': (dict(refine_net_rnn_type='CGRU'), True),
    'lstm-crnn': (dict(eye_net_rnn_type='LSTM', refine_net_rnn_type='CRNN'), False),
    'clstm': (dict(refine_net_rnn_type='CLSTM', refine_net_clstm_feeds_features=False), False),
    'clstm-live': (dict(refine_net_rnn_type='CLSTM', refine_net_clstm_feeds_features=True), False),
    'cgru-x2-w32': (dict(refine_net_rnn_type='CGRU', refine_net_rnn_num_cells=2, refine_net_num_features=32), False),
}
# one T = 10 clip, three streams, steps of Tc = 4: per step the frames each stream consumes.  Stream 0 runs ahead and then idles,
# stream 1 has a step without frames in the middle, stream 2 trickles; the last step is partial for the streams still running.
T_CLIP, TC = 10, 4
PACES = [[4, 2, 1], [4, 0, 3], [2, 4, 2], [0, 4, 4]]
assert all(sum(p[b] for p in PACES) == T_CLIP for b in range(3))


class RaggedFakes(StreamFakes):
    """StreamFakes plus include/eve_hip.h eve_stream_state_rows_at and eve_eye_tail_stream_fwd_len."""

    def stream_state_rows_at(self, src, dst, lengths):
        self.calls.append('stream_state_rows_at')
        for s in range(dst.shape[0]):
            n = min(int(lengths[s]), src.shape[1])
            if n > 0:
                dst[s].copy_(src[s, n - 1])
        return dst

    def eye_tail_stream_fwd_len(self, feats, head_pose, weights, h, lengths, reset=None, want_hs=False):
        before = h.clone()
        gaze, pupil, hs = self.eye_tail_stream_fwd(feats, head_pose, weights, h, reset, want_hs=True)
        self.calls[-1] = 'eye_tail_stream_fwd_len'
        for s in range(h.shape[0]):
            n = min(max(int(lengths[s]), 0), hs.shape[1])
            if n > 0:
                h[s].copy_(hs[s, n - 1])
            else:
                h[s].copy_(torch.zeros_like(before[s]) if reset is not None and int(reset[s]) != 0 else before[s])
        return gaze, pupil, (hs if want_hs else None)


class LoggingFakes(RaggedFakes):
    """Records every stand-in kernel call as (name, the shapes and dtypes of its tensor arguments)."""

    def __init__(self):
        RaggedFakes.__init__(self)
        self.log = []

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name.startswith('_') or not callable(attr) or isinstance(attr, type):
            return attr
        log = object.__getattribute__(self, 'log')

        def describe(v):
            if torch.is_tensor(v):
                return [[list(v.shape), str(v.dtype)]]
            if isinstance(v, (tuple, list)):
                return [d for x in v for d in describe(x)]
            return []

        def wrapped(*args, **kwargs):
            log.append([name, describe(args) + describe([kwargs[k_] for k_ in sorted(kwargs)])])
            return attr(*args, **kwargs)
        return wrapped


@pytest.fixture()
def fake():
    k = RaggedFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def make_model(over, fused=False):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'refine_net.json'))
    cfg.import_dict(dict(eye_net_load_pretrained=False, **over))
    model = eve_amd.EVE(output_predictions=True)
    detweights.fill_module(model.eye_net, 0)
    detweights.fill_module(model.refine_net, 1)
    model.eye_net.compute_dtype = model.refine_net.compute_dtype = torch.float32
    model.eye_net.stream_fused_tail = fused
    return model.eval()


def padded_chunk(batch, starts, Tc, seed):
    """A [B, Tc, ...] chunk whose stream b holds the clip's frames starts[b] .. starts[b] + Tc - 1, and seeded random finite
    values of the input's own dtype where the clip has no such frame."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in chunk_of(batch, 0, batch['left_eye_patch'].shape[1]).items():
        T = v.shape[1]
        rows = []
        for b, t0 in enumerate(starts):
            have = v[b, t0:min(T, t0 + Tc)]
            shape = (Tc - have.shape[0],) + tuple(v.shape[2:])
            if v.dtype == torch.uint8:
                pad = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
            else:
                pad = torch.randn(shape, generator=g).to(v.dtype)
            rows.append(torch.cat([have, pad], dim=0))
        out[k] = torch.stack(rows, dim=0).contiguous()
    return out


def run_paces(stream, batch, paces, Tc, seed=11):
    """Consume the clip at the given paces; -> per key the [B, T, ...] concatenation of every stream's valid outputs."""
    B = len(paces[0])
    pos, parts = [0] * B, [[] for _ in range(B)]
    for i, n in enumerate(paces):
        out = stream.step(padded_chunk(batch, pos, Tc, seed + i), lengths=list(n))
        valid = out.pop('valid')
        assert valid.dtype == torch.bool and tuple(valid.shape) == (B, Tc)
        assert valid.cpu().tolist() == [[t < n[b] for t in range(Tc)] for b in range(B)]
        for b in range(B):
            parts[b].append({k: v[b, :n[b]].clone() for k, v in out.items()})
            pos[b] += n[b]
    return {k: torch.stack([torch.cat([p[k] for p in parts[b]], dim=0) for b in range(B)], dim=0) for k in parts[0][0]}


def flat_state(st):
    return [(k, i, t) for k in sorted(st) for i, t in enumerate(st[k] if isinstance(st[k], tuple) else (st[k],))]


# ------------------------------------------------------------------------------------------------ arguments and the mask
def test_lengths_are_validated(fake):
    model = make_model(dict(refine_net_rnn_type='CGRU'))
    s = eve_amd.EVEStream(model, 2, use_graph=False)
    ch = chunk_of(clip(2, 3, seed=5), 0, 3)
    for bad in ([1], [1, 2, 3], [-1, 2], [1, 4], [1.0, 2.0], np.array([1.0, 2.0]), torch.tensor([1.0, 2.0]), [[1, 2]]):
        with pytest.raises(ValueError):
            s.step(ch, lengths=bad)
    assert not fake.calls                                         # a refused step has launched nothing
    for good in ([3, 0], np.array([1, 2]), torch.tensor([0, 0]), np.array([2, 3], dtype=np.uint8)):
        s.step(ch, lengths=good)


def test_valid_mask_only_with_lengths(fake):
    model = make_model(dict(refine_net_rnn_type='CGRU'))
    s = eve_amd.EVEStream(model, 3, use_graph=False)
    ch = chunk_of(clip(3, 4, seed=5), 0, 4)
    plain = s.step(ch)
    assert 'valid' not in plain
    out = s.step(ch, lengths=[4, 0, 2])
    assert out['valid'].dtype == torch.bool
    assert out['valid'].tolist() == [[True] * 4, [False] * 4, [True, True, False, False]]
    assert set(out) == set(plain) | {'valid'}
    for k, v in plain.items():
        assert out[k].shape == v.shape, k
    assert 'valid' not in s.step(ch)


# ------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_ragged_split_matches_the_whole_clip(fake, name):
    """Three streams consume one 10-frame clip at different paces (steps of 4 frames, one stream idle in one step, a partial last
    step, random values in the frames nobody delivered): every stream's valid outputs, concatenated, equal the whole-clip eval
    pass within test_stream_host.tol -- a ragged split is a split -- and the carried states afterwards equal those of the
    uniform run of the same frames."""
    over, fused = CONFIGS[name]
    model = make_model(over, fused)
    batch = clip(3, T_CLIP, seed=9)
    ragged = eve_amd.EVEStream(model, 3, use_graph=False)
    got = run_paces(ragged, batch, PACES, TC)
    assert ('eye_tail_stream_fwd_len' in fake.calls) == fused and 'stream_state_rows_at' in fake.calls
    assert 'eye_tail_stream_fwd' not in fake.calls
    with torch.no_grad():
        whole = model(dict(batch))
    checked = 0
    for k, v in got.items():
        if k in whole:
            checked += 1
            assert float((v - whole[k]).abs().max()) < tol(k), k
    assert checked >= 6
    uniform = eve_amd.EVEStream(model, 3, use_graph=False)
    for t0 in (0, 4, 8):
        uniform.step(chunk_of(batch, t0, min(T_CLIP, t0 + 4)))
    for (k, i, a), (_, _, b) in zip(flat_state(ragged.get_state()), flat_state(uniform.get_state())):
        # EyeNet's states feed the initial gaze and carry its bound; RefineNet's sit behind the heat-map of that gaze, on the path
        # of the refined keys, and carry theirs (test_stream_host.tol's amplification)
        assert float((a - b).abs().max()) < tol('g_final' if k.startswith('refinenet') else 'g_initial'), (k, i)


def test_reset_reaches_a_stream_without_frames(fake):
    model = make_model(dict(refine_net_rnn_type='CLSTM'))
    batch = clip(2, 6, seed=7)
    s = eve_amd.EVEStream(model, 2, use_graph=False)
    s.step(chunk_of(batch, 0, 3))
    before = flat_state(s.get_state())
    s.reset([1])
    s.step(chunk_of(batch, 3, 6), lengths=[0, 0])
    for (k, i, a), (_, _, b) in zip(flat_state(s.get_state()), before):
        assert torch.equal(a[0], b[0]), k                         # stream 0: no frames, no reset -- untouched
        assert not a[1].any() and b[1].any(), k                   # stream 1: zero state


# ------------------------------------------------------------------------------------------------ uniform steps are untouched
UNIFORM_CASES = [('gru-cgru', [3, 1]), ('gru-cgru-fused-tail', [2]), ('lstm-crnn', [2]), ('clstm-live', [2])]


def record_uniform_calls():
    """The stand-in kernel calls of uniform steps (with a reset before the second one), per case of UNIFORM_CASES.  The
    committed tests/golden/stream_uniform_calls.json is this function's result on the commit before ragged steps."""
    rec = {}
    for name, sizes in UNIFORM_CASES:
        over, fused = CONFIGS[name]
        k = LoggingFakes()
        kernels.set_default_kernels(k)
        try:
            model = make_model(over, fused)
            batch = clip(2, sum(sizes), seed=3)
            s = eve_amd.EVEStream(model, 2, use_graph=False)
            t0 = 0
            for i, n in enumerate(sizes):
                if i:
                    s.reset([1])
                s.step(chunk_of(batch, t0, t0 + n))
                t0 += n
        finally:
            kernels.set_default_kernels(None)
            eve_amd.reset_standalone_config()
        rec[name] = k.log
    return rec


def test_uniform_steps_issue_the_calls_they_always_did():
    want = json.load(open(GOLDEN_CALLS))
    got = json.loads(json.dumps(record_uniform_calls()))
    assert sorted(got) == sorted(want)
    for name in want:
        names = [c[0] for c in got[name]]
        assert 'stream_state_rows_at' not in names and 'eye_tail_stream_fwd_len' not in names, name
        assert len(got[name]) == len(want[name]), name
        for i, (a, b) in enumerate(zip(got[name], want[name])):
            assert a == b, (name, i, a, b)
    # the recorder sees the ragged calls when there are some
    k = LoggingFakes()
    kernels.set_default_kernels(k)
    try:
        eve_amd.EVEStream(make_model(*CONFIGS['gru-cgru']), 2, use_graph=False).step(chunk_of(clip(2, 2, seed=3), 0, 2), lengths=[1, 2])
    finally:
        kernels.set_default_kernels(None)
        eve_amd.reset_standalone_config()
    assert 'stream_state_rows_at' in [c[0] for c in k.log]
