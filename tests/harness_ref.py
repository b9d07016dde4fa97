"""float64 references, case grids and comparison helpers for everything EVE.forward and the train step do around the two
networks: eve_amd/csrc/gaze_geometry.hip, heatmap_loss.hip, losses.hip and the sumsq / Adam kernels of optim.hip, with their
autograd shells in eve_amd/ops.py and eve_amd/losses.py.  tests/test_gpu_harness_f64.py runs the helpers on the HIP kernels,
tests/test_harness_ref_host.py on the float32 CPU restatement (and on copies of it with one planted defect each).  CPU only.

References
  * geometry, heat-maps, soft-argmax: the oracle's functions (oracle/eve.py) on float64 tensors; Jacobians and backwards by
    float64 autograd.
  * heat-map head and losses: the documented contract of heatmap_loss.hip in float64 (log terms clamped at -100, BCE gradient
    (p - g) / max(p (1 - p), 1e-12), a clip's sum divided by its number of valid frames only when that exceeds one).
  * vector terms and eye losses: the formulas of losses.hip's header in float64, with the contract's float32 semantics: the
    cosine clamp limit 1 - 1e-8 IS 1.0, the gradient is zero where the clamp is active (torch gives NaN), sign(0) = 0.
  * Adam: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(weight_decay=...) on float64 copies, lr / beta / eps / wd rounded
    to float32 first (the C ABI takes floats); the guard's bookkeeping as plain Python (GuardBook).

The comparison rule (judge / judge_rows): the yardstick of a tensor is the error of the float32 CPU restatement (Restatement:
FakeKernels plus the float32 tensor expressions of eve_amd/losses.py) against float64 ON THE SAME OPERANDS, floored at 2^-24 of
the tensor's scale; the kernel's error may be at most MARGIN = 4 times that.  Derived bounds replace it in two places: sumsq
(sumsq_chain) and the per-row bound of gaze_to_pog's values (POG_ROW_REL).  Over more than 256 clips the restatement adds
the clip means of a vector term in float32 in clip order, as vector_terms_kernel does (Restatement.clip_sum), so that the
yardstick carries the rounding of that order and not of a pairwise mean().  Row-wise comparisons choose the row's scale from the float64
reference: gaze_to_pog rows by |mm| + |J|, angular gradient rows by their sensitivity to the cosine (angular_row_scale),
the heat-map loss gradient element by element.
"""
import functools
import math

import numpy as np
import torch

from fake_kernels import FakeKernels
from oracle import detweights
from oracle import eve as oe
from oracle.config import OracleConfig

F64 = torch.float64
EPS = 2.0 ** -24
MARGIN = 4.0
SCREEN = (1920, 1080)
DEG = 180.0 / math.pi


def HERE(t):
    """`put` of a stand-in that computes on the CPU"""
    return t


# ------------------------------------------------------------------------------------------------ the float32 restatement
class Restatement(FakeKernels):
    """FakeKernels plus float32 statements of vector_terms / eye_losses: the tensor expressions of eve_amd/losses.py (the ones
    the kernels replaced) under float32 autograd.  The yardstick of every comparison below."""
    name = 'float32-restatement'
    SEQUENTIAL_CLIPS = 256

    @staticmethod
    def per_step(kind, p, q):
        """[B, T, D] -> [B, T]: the per-step expressions of eve_amd/losses.py"""
        from eve_amd import losses
        if kind == 'mse':
            return losses._per_step((p - q) ** 2)
        if kind == 'euclidean':
            return torch.sqrt(((p - q) ** 2).flatten(2).sum(dim=2))
        if kind == 'l1':
            return losses._per_step((p - q).abs())
        cos = torch.nn.functional.cosine_similarity(losses.gaze_vectors(p), losses.gaze_vectors(q), dim=-1, eps=1e-8)
        return torch.acos(torch.nn.functional.hardtanh(cos, min_val=-1 + 1e-8, max_val=1 - 1e-8)) * DEG

    def clip_sum(self, clip_means):
        """The clip means added in float32 one after the other in clip order (numpy's cumsum does exactly that; torch's sum()
        adds pairwise and its cumsum accumulates float in double): what one thread of vector_terms_kernel does."""
        return torch.tensor(np.cumsum(clip_means.numpy(), dtype=np.float32)[-1])

    def vector_terms(self, items, want_grad):
        """Values and gradients of the tensor expressions.  Above SEQUENTIAL_CLIPS clips the VALUE is the ordered float32 sum
        of the float32 clip means over B: the rounding of a sequential sum grows with its length (about 0.3 sqrt(B) spacings,
        20 at B = 4096, against one or two for a pairwise sum), and a yardstick has to carry the rounding of the order it is a
        yardstick for."""
        from eve_amd import losses
        fns = {'mse': losses.mse_loss, 'euclidean': losses.euclidean_loss, 'l1': losses.l1_loss, 'angular': losses.angular_loss}
        out, dps = [], []
        for (kind, pred, tgt, val), wg in zip(items, want_grad):
            assert not (wg and kind == 'euclidean')
            B, T = val.shape
            with torch.enable_grad():
                p = pred.detach().clone().requires_grad_(True)
                v = fns[kind](p.reshape(B, T, -1), tgt.reshape(B, T, -1), val)
                dps.append(torch.nan_to_num(torch.autograd.grad(v, p)[0], nan=0.0, posinf=0.0, neginf=0.0) if wg else None)
            v = v.detach()
            if B > self.SEQUENTIAL_CLIPS:
                m = val.float()
                n = m.sum(dim=1)
                means = (self.per_step(kind, pred.reshape(B, T, -1), tgt.reshape(B, T, -1)) * m).sum(dim=1) / torch.where(n > 1, n, torch.ones_like(n))
                v = self.clip_sum(means) / torch.tensor(float(B))
            out.append(v)
        return torch.stack(out), dps

    def eye_losses(self, g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, coeff_ang, coeff_l1):
        if p_pred[0].shape[1] > 256:
            raise RuntimeError('eye_losses: bad arguments (T <= 256)')
        terms, dg, dp = [], [], []
        for s in range(2):
            o, d = self.vector_terms([('angular', g_pred[s], g_tgt[s], g_val[s]), ('l1', p_pred[s], p_tgt[s], p_val[s])], [True, True])
            terms += [o[0], o[1]]
            dg.append(d[0]); dp.append(d[1])
        full = coeff_ang * (terms[0] + terms[2]) + coeff_l1 * (terms[1] + terms[3])
        return torch.stack(terms + [full]), dg, dp


BASE = Restatement()


# ------------------------------------------------------------------------------------------------ comparison
def c64(t):
    return t.detach().cpu().to(F64)


def _note(rec, key, what, err, yard):
    ratio = err / yard
    print('%-58s err %.3e  yardstick %.3e  ratio %.2f' % (what, err, yard, ratio))
    if rec is not None:
        rec[key] = max(rec.get(key, 0.0), ratio)
    assert ratio <= MARGIN, '%s: error %.3e is %.2f x the float32 restatement\'s %.3e' % (what, err, ratio, yard)
    return ratio


def judge(rec, key, what, got, want, base, scale=None):
    """max|got - want| against max(max|base - want|, 2^-24 scale); scale: max|want| unless given."""
    got, want, base = c64(got), c64(want), c64(base)
    assert got.shape == want.shape == base.shape, (what, got.shape, want.shape, base.shape)
    assert bool(torch.isfinite(got).all()), '%s: not finite' % what
    s = float(want.abs().max()) if scale is None else float(scale)
    s = max(s, 1e-30)
    return _note(rec, key, what, float((got - want).abs().max()), max(float((base - want).abs().max()), EPS * s))


def rows_err(x, want, row_scale):
    e = (c64(x) - want).abs().reshape(want.shape[0], -1).max(dim=1).values
    return float((e / row_scale).max())


def judge_rows(rec, key, what, got, want, base, row_scale):
    """The same rule with one scale per row (first dimension): max_n |got - want|_n / scale_n against the restatement's."""
    want = c64(want)
    assert bool(torch.isfinite(c64(got)).all()), '%s: not finite' % what
    row_scale = row_scale.clamp_min(1e-300)
    return _note(rec, key, what, rows_err(got, want, row_scale), max(rows_err(base, want, row_scale), EPS))


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def uni(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def cfg_for(hw, screen=SCREEN):
    c = OracleConfig()
    c.gaze_heatmap_size = [hw[1], hw[0]]
    c.actual_screen_size = [screen[0], screen[1]]
    return c


# ------------------------------------------------------------------------------------------------ gaze_to_pog / combined_gaze
POG_N = (1, 127, 128, 129, 300)        # one thread; either side of one 128-thread workgroup; three workgroups
POG_SEED = 11
# Worst row of the float32 restatement over POG_N x (plain, kappa): max |mm32 - mm64| / (|mm64|_inf + |d mm64 / d g|_inf),
# measured by test_harness_ref_host.py::test_the_per_row_bound_of_gaze_to_pog_is_the_restatements_worst_row (which holds this
# figure between the measurement and 1.5 x it).  A kernel's rows may be MARGIN x this.
POG_ROW_REL = 2.5e-7


@functools.lru_cache(maxsize=None)
def frames(N, seed=POG_SEED):
    """Flat geometry operands of N frames from the synthetic clip generator; pitch ~ 0.36 N(0, 1), yaw ~ 0.56 N(0, 1): about
    half the rays leave the screen on each axis (the host test holds 30 % .. 70 % on-screen), some graze the screen plane.
    Shared between the checks: never modified."""
    b = detweights.eve_batch(N, 1, seed=seed)
    g = torch.Generator().manual_seed(seed)
    return {'g': 0.4 * torch.randn(N, 2, generator=g) * torch.tensor([0.9, 1.4]), 'kappa': 0.05 * torch.randn(N, 2, generator=g),
            'o': b['left_o'].reshape(N, 3), 'R': b['left_R'].reshape(N, 3, 3), 'head_R': b['head_R'].reshape(N, 3, 3),
            'inv': b['inv_camera_transformation'].reshape(N, 4, 4), 'cam': b['camera_transformation'].reshape(N, 4, 4),
            'ppm': b['pixels_per_millimeter'].reshape(N, 2)}


def pog_f64(f, augment, g=None):
    """oracle geometry on float64 operands -> dict(g_out, mm, px, jac [N, 6, 2], raw px before the clamp, on [N, 2] bool)."""
    d = {k: v.to(F64) for k, v in f.items()}
    gi = (d['g'] if g is None else g.to(F64)).clone().requires_grad_(True)
    go = oe.offset_augmentation(gi, d['head_R'], d['kappa']) if augment else gi
    mm, px = oe.to_screen_coordinates(d['o'], go, d['R'], d['inv'], d['ppm'], SCREEN)
    jac = torch.zeros(gi.shape[0], 6, 2, dtype=F64)
    for oi, o in enumerate((go, mm, px)):
        for c in range(2):
            if o is gi:
                jac[:, 2 * oi + c, c] = 1.0
            else:
                jac[:, 2 * oi + c] = torch.autograd.grad(o[:, c].sum(), gi, retain_graph=True)[0]    # frames are independent
    raw = mm.detach() * d['ppm']
    on = torch.stack([(raw[:, 0] >= 0) & (raw[:, 0] <= SCREEN[0]), (raw[:, 1] >= 0) & (raw[:, 1] <= SCREEN[1])], dim=1)
    return dict(g_out=go.detach(), mm=mm.detach(), px=px.detach(), jac=jac, raw=raw, on=on, ppm=d['ppm'])


@functools.lru_cache(maxsize=None)
def pog_reference(N, augment):
    f = frames(N)
    return f, pog_f64(f, augment)


def run_pog(k, f, augment, mv):
    out = k.gaze_to_pog(mv(f['g']), mv(f['o']), mv(f['R']), mv(f['inv']), mv(f['ppm']), SCREEN,
                        mv(f['head_R']) if augment else None, mv(f['kappa']) if augment else None)
    return [t.detach().cpu() for t in out]


@functools.lru_cache(maxsize=None)
def pog_base(N, augment):
    return run_pog(BASE, frames(N), augment, HERE)


def block_norms(jac):
    """|.|_inf of the three 2 x 2 blocks (g_out, mm, px) per row -> [N, 3]"""
    return jac.abs().reshape(jac.shape[0], 3, 4).max(dim=2).values


def pog_row_scale(want):
    return want['mm'].abs().max(dim=1).values + block_norms(want['jac'])[:, 1]


def pog_row_error(mm, want):
    return float(((c64(mm) - want['mm']).abs().max(dim=1).values / pog_row_scale(want)).max())


def check_gaze_to_pog(k, N, augment, put, rec=None, base=BASE):
    """Values, all twelve Jacobian entries, exact zeros in the px rows of off-screen axes."""
    f, want = pog_reference(N, augment)
    what = 'gaze_to_pog N%d %s ' % (N, 'kappa' if augment else 'plain')
    g_out, mm, px, jac = run_pog(k, f, augment, put)
    b_g, b_mm, b_px, b_jac = pog_base(N, augment) if base is BASE else run_pog(base, f, augment, HERE)
    on, scale = want['on'], pog_row_scale(want)
    if augment:
        judge(rec, 'gaze_to_pog g_out', what + 'g_out', g_out, want['g_out'], b_g)
    else:
        assert torch.equal(g_out, f['g']), what + 'g_out is g itself'
    err = pog_row_error(mm, want)
    print('%-58s err %.3e  restatement %.3e  bound %.3e' % (what + 'mm (per row)', err, pog_row_error(b_mm, want), MARGIN * POG_ROW_REL))
    if rec is not None:
        rec['gaze_to_pog mm / bound'] = max(rec.get('gaze_to_pog mm / bound', 0.0), err / (MARGIN * POG_ROW_REL))
    assert err <= MARGIN * POG_ROW_REL, what + 'mm: a row is off by %.3e of |mm| + |J|' % err
    px_err = ((c64(px) - want['px']).abs() / (scale[:, None] * want['ppm']))[on]
    assert px_err.numel() == 0 or float(px_err.max()) <= MARGIN * POG_ROW_REL, what + 'px on-screen: %.3e' % float(px_err.max())
    assert torch.equal(c64(px)[~on], want['px'][~on]), what + 'px of an off-screen axis is not the clamp value'
    nb = block_norms(want['jac'])
    if augment:
        judge_rows(rec, 'gaze_to_pog jac', what + 'jac g_out', jac[:, 0:2], want['jac'][:, 0:2], b_jac[:, 0:2], nb[:, 0])
    else:
        assert torch.equal(jac[:, 0:2], torch.eye(2).expand(N, 2, 2)), what + 'd g_out / d g is the identity'
    judge_rows(rec, 'gaze_to_pog jac', what + 'jac mm', jac[:, 2:4], want['jac'][:, 2:4], b_jac[:, 2:4], nb[:, 1])
    judge_rows(rec, 'gaze_to_pog jac', what + 'jac px', jac[:, 4:6], want['jac'][:, 4:6], b_jac[:, 4:6],
               nb[:, 1] * want['ppm'].max(dim=1).values)
    for a in range(2):
        assert bool((jac[:, 4 + a][~on[:, a]] == 0).all()), what + 'jac px row %d of an off-screen axis is not exactly 0' % a
    return jac


def check_gaze_to_pog_bwd(k, N, augment, put, rec=None, base=BASE):
    """The eight present / absent combinations of (dg_out, dmm, dpx) on the float64 Jacobians rounded to float32, then all three
    chained on the kernel's own Jacobians against the float64 ones."""
    f, want = pog_reference(N, augment)
    what = 'gaze_to_pog_bwd N%d %s ' % (N, 'kappa' if augment else 'plain')
    d = [rnd((N, 2), 70 + i) for i in range(3)]
    jac32 = want['jac'].float()

    def ref(jac, present):
        return sum(torch.einsum('ni,nij->nj', d[i].to(F64), jac[:, 2 * i:2 * i + 2]) for i in range(3) if present[i])

    def scale(jac, present):
        nb = block_norms(jac)
        return sum(d[i].to(F64).abs().max(dim=1).values * nb[:, i] for i in range(3) if present[i])
    for mask in range(8):
        present = [bool(mask >> i & 1) for i in range(3)]
        args = lambda mv: [mv(d[i]) if present[i] else None for i in range(3)]
        got = k.gaze_to_pog_bwd(put(jac32), *args(put))
        if mask == 0:
            assert bool((got == 0).all()), what + 'no upstream gradient -> zeros'
            continue
        judge_rows(rec, 'gaze_to_pog_bwd', what + ''.join('gmp'[i] if present[i] else '-' for i in range(3)), got,
                   ref(jac32.to(F64), present), base.gaze_to_pog_bwd(jac32, *args(HERE)), scale(jac32.to(F64), present))
    own = k.gaze_to_pog(put(f['g']), put(f['o']), put(f['R']), put(f['inv']), put(f['ppm']), SCREEN,
                        put(f['head_R']) if augment else None, put(f['kappa']) if augment else None)[3]
    b_jac = pog_base(N, augment)[3] if base is BASE else run_pog(base, f, augment, HERE)[3]
    judge_rows(rec, 'gaze_to_pog_bwd', what + 'chained', k.gaze_to_pog_bwd(own, *[put(t) for t in d]), ref(want['jac'], [True] * 3),
               base.gaze_to_pog_bwd(b_jac, *d), scale(want['jac'], [True] * 3))


@functools.lru_cache(maxsize=None)
def combined_reference(N):
    f = frames(N)
    pog = torch.stack([uni((N,), 31) * 553, uni((N,), 32) * 311], dim=1)
    d = {k: v.to(F64) for k, v in f.items()}
    g = oe.combined_gaze_direction(d['o'], pog.to(F64), d['R'], d['cam'])
    return f, pog, g, pog_f64(f, False, g=g)


def check_combined_gaze(k, N, put, rec=None, base=BASE):
    """combined_gaze against float64, and its round trip through gaze_to_pog (the same frame, plain) back to the point."""
    f, pog, want_g, rt = combined_reference(N)
    what = 'combined_gaze N%d ' % N
    run = lambda kk, mv: kk.combined_gaze(mv(f['o']), mv(pog), mv(f['R']), mv(f['cam']))
    got, bas = run(k, put), run(base, HERE)
    judge(rec, 'combined_gaze', what + 'g', got, want_g, bas)
    back = lambda kk, mv, g: kk.gaze_to_pog(g.contiguous(), mv(f['o']), mv(f['R']), mv(f['inv']), mv(f['ppm']), SCREEN)[1]
    judge_rows(rec, 'combined_gaze round trip', what + 'round trip mm', back(k, put, got), rt['mm'], back(base, HERE, bas), pog_row_scale(rt))


# ------------------------------------------------------------------------------------------------ heat-maps / soft-argmax
HEAT_HW = ((2, 2), (5, 7), (33, 31), (17, 61), (72, 128))      # smallest legal; H W < 256 (idle lanes); odd, > 1024 px; the real map
HEAT_N = (1, 37)
SIGMAS = (10.0, 3.0, 0.7)
CHUNK_N = 65539                                                # 65 535 + 4: the wrappers' second chunk


def heat_case(H, W, N, seed=0):
    """centres [N, 2] px: row 0 exactly on a pixel, rows 1 / 2 (N > 2) far off-screen, the rest anywhere within 100 px of the
    screen; validity with row 0 valid and row 1 invalid; an upstream gradient."""
    s = 1000 * H + 10 * W + N + seed
    c = torch.stack([uni((N,), s) * 2120 - 100, uni((N,), s + 1) * 1280 - 100], dim=1)
    c[0] = torch.tensor([(W // 2) * SCREEN[0] / W, (H // 2) * SCREEN[1] / H])
    if N > 2:
        c[1] = torch.tensor([-300.0, 500.0])
        c[2] = torch.tensor([2500.0, 1500.0])
    valid = uni((N,), s + 2) > 0.3
    valid[0] = True
    if N > 1:
        valid[1] = False
    return c, valid, rnd((N, 1, H, W), s + 3)


def heat_f64(c, sigma, hw, dout=None):
    ci = c.to(F64).clone().requires_grad_(True)
    m = oe.make_heatmaps(ci, sigma, cfg_for(hw))
    return m.detach(), (None if dout is None else torch.autograd.grad((m * dout.to(F64)).sum(), ci)[0])


def check_make_heatmaps(k, H, W, N, sigma, put, rec=None, base=BASE):
    c, valid, dout = heat_case(H, W, N)
    what = 'make_heatmaps %dx%d N%d sigma %g ' % (H, W, N, sigma)
    want, want_d = heat_f64(c, sigma, (H, W), dout)
    got = k.make_heatmaps(put(c), sigma, (H, W), SCREEN)
    assert tuple(got.shape) == (N, 1, H, W)
    judge(rec, 'make_heatmaps', what, got, want, base.make_heatmaps(c, sigma, (H, W), SCREEN), scale=1.0)
    masked = k.make_heatmaps(put(c), sigma, (H, W), SCREEN, validity=put(valid)).cpu()
    assert bool((masked[~valid] == 0).all()), what + 'an invalid map is not exactly 0'
    assert torch.equal(masked[valid], got.cpu()[valid]), what + 'a valid map changed under the mask'
    judge(rec, 'make_heatmaps_bwd', what + 'bwd', k.make_heatmaps_bwd(put(c), sigma, SCREEN, put(dout)), want_d,
          base.make_heatmaps_bwd(c, sigma, SCREEN, dout))


def soft_maps(H, W, N):
    """N == 1: one low, broad Gaussian towards the far corner (softmax(100 h) spreads over the map, so the whole grid and every
    pixel's gradient count).  Otherwise row 0 flat, rows 1-4 a single spike in each corner, row 5 a near-saturated
    sigmoid-like map (values ~0 / ~1, a rectangle of ones), the rest noisy Gaussians as test_gpu_eve.py draws them."""
    s = 2000 * H + 10 * W + N
    c = torch.stack([uni((N,), s) * SCREEN[0], uni((N,), s + 1) * SCREEN[1]], dim=1)
    heat = oe.make_heatmaps(c, max(5.0 * W / 128, 0.7), cfg_for((H, W))) * 0.9 + 0.05 * uni((N, 1, H, W), s + 2)
    if N == 1:
        heat = oe.make_heatmaps(torch.tensor([[0.8 * SCREEN[0], 0.7 * SCREEN[1]]]), 0.4 * W, cfg_for((H, W))) * 0.03 + 0.005 * uni((1, 1, H, W), s + 2)
    else:
        heat[0].zero_()
        heat[1:5].zero_()
        for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
            heat[1 + i, 0, y, x] = 5.0
        m = -torch.ones(H, W)
        m[H // 3:H // 3 + max(H // 3, 1), W // 4:W // 4 + max(W // 2, 1)] = 1.0
        heat[5, 0] = torch.sigmoid(15.0 * m + rnd((H, W), s + 3))
    return heat, rnd((N, 2), s + 4)


CORNERS = torch.tensor([[0.0, 0.0], [SCREEN[0], 0.0], [0.0, SCREEN[1]], [SCREEN[0], SCREEN[1]]])


def soft_f64(heat, dpog):
    """-> px, d heat, stats [N, 4] = lx, ly, max(100 h), sum exp(100 h - max) as the forward kernel stores them"""
    N, _, H, W = heat.shape
    hi = heat.to(F64).clone().requires_grad_(True)
    px = oe.soft_argmax(hi, cfg_for((H, W)))
    dh = torch.autograd.grad((px * dpog.to(F64)).sum(), hi)[0]
    z = 100.0 * heat.to(F64).reshape(N, -1)
    mx = z.max(dim=1).values
    e = torch.exp(z - mx[:, None])
    xs = (torch.arange(W, dtype=F64) / (W - 1)).repeat(H)
    ys = (torch.arange(H, dtype=F64) / (H - 1)).repeat_interleave(W)
    stats = torch.stack([(e * xs).sum(1) / e.sum(1), (e * ys).sum(1) / e.sum(1), mx, e.sum(1)], dim=1)
    return px.detach(), dh, stats


def check_soft_argmax(k, H, W, N, put, rec=None, base=BASE, heat=None, dpog=None):
    if heat is None:
        heat, dpog = soft_maps(H, W, N)
    N = heat.shape[0]
    what = 'soft_argmax %dx%d N%d ' % (H, W, N)
    want, want_d, stats64 = soft_f64(heat, dpog)
    dheat = put(heat)
    got, stats = k.soft_argmax_fwd(dheat, SCREEN)
    bas = base.soft_argmax_fwd(heat, SCREEN)[0]
    for a in range(2):
        judge(rec, 'soft_argmax_fwd', what + 'px ' + 'xy'[a], got[:, a], want[:, a], bas[:, a], scale=SCREEN[a])
    if N >= 6 and heat.shape[0] == N and bool((heat[1:5].sum(dim=(1, 2, 3)) == 5.0).all()):
        assert torch.equal(got[1:5].cpu(), CORNERS), what + 'a corner spike does not give the corner: %s' % got[1:5].cpu().tolist()
    bas_d = base.soft_argmax_bwd(heat, None, dpog, SCREEN)
    own = k.soft_argmax_bwd(dheat, stats, put(dpog), SCREEN)
    judge(rec, 'soft_argmax_bwd', what + 'bwd on its own stats', own, want_d, bas_d)
    judge(rec, 'soft_argmax_bwd', what + 'bwd on float64 stats', k.soft_argmax_bwd(dheat, put(stats64.float()), put(dpog), SCREEN),
          want_d, bas_d)


def check_chunked_maps(k, put, rec=None, base=BASE, n=CHUNK_N):
    """65 539 maps of 2 x 2 through the two wrappers that launch at most 65 535 maps at a time.  Every map has its own centre
    and its own upstream gradient, so a chunk that read another chunk's rows would be wrong everywhere."""
    c = torch.stack([uni((n,), 91) * SCREEN[0], uni((n,), 92) * SCREEN[1]], dim=1)
    valid = uni((n,), 93) > 0.2
    got = k.make_heatmaps(put(c), 0.7, (2, 2), SCREEN, validity=put(valid))
    want = heat_f64(c, 0.7, (2, 2))[0] * valid.to(F64).view(-1, 1, 1, 1)
    judge(rec, 'make_heatmaps', 'make_heatmaps 2x2 N%d (two chunks) ' % n, got, want,
          base.make_heatmaps(c, 0.7, (2, 2), SCREEN, validity=valid), scale=1.0)
    heat = (want + 0.05 * uni((n, 1, 2, 2), 94).to(F64)).float()
    check_soft_argmax(k, 2, 2, n, put, rec, base, heat=heat, dpog=rnd((n, 2), 95))


# ------------------------------------------------------------------------------------------------ the heat-map head
HEAD_PIXELS = (1, 257, 2 * 8192 * 256 + 77)                    # one thread; two workgroups; a second grid-stride turn plus a tail
HEAD_CASES = [(dt, 8, P) for dt in (torch.float32, torch.bfloat16, torch.float16) for P in HEAD_PIXELS[:2]] + \
             [(torch.float32, 4, P) for P in HEAD_PIXELS[:2]] + [(torch.bfloat16, 8, HEAD_PIXELS[2])]


def head_logits(dtype, cpad, P):
    big = float(torch.finfo(dtype).max)
    x = rnd((1, 1, P, cpad), 7 * P + cpad, 4.0)
    special = torch.tensor([0.0, 20.0, -20.0, 90.0, -90.0, big, -big])
    m = min(P, special.numel())
    x[0, 0, P - m:, 0] = special[:m]                           # at the END: the last pixels of the last turn
    return x.to(dtype)


def check_head(k, dtype, cpad, P, put, rec=None, base=BASE):
    what = 'heatmap_head %s Cpad %d P%d ' % (str(dtype).split('.')[-1], cpad, P)
    logits = head_logits(dtype, cpad, P)
    want = torch.sigmoid(logits[..., 0].to(F64)).unsqueeze(1)
    got = k.heatmap_head_fwd(put(logits))
    assert tuple(got.shape) == (1, 1, 1, P) and got.dtype == torch.float32
    g = got.cpu()
    assert bool(torch.isfinite(g).all()) and bool(((g >= 0) & (g <= 1)).all()), what + 'leaves [0, 1]'
    judge(rec, 'heatmap_head_fwd', what + 'fwd', got, want, base.heatmap_head_fwd(logits), scale=1.0)
    y, dy = want.float(), rnd((1, 1, 1, P), 3 * P + 1)
    dl = k.heatmap_head_bwd(put(dy), put(y), dtype, cpad)
    assert dl.dtype == dtype and tuple(dl.shape) == (1, 1, P, cpad)
    assert bool((dl[..., 1:] == 0).all()), what + 'a padding channel of dlogits is not exactly 0'
    want_d = (dy.to(F64) * y.to(F64) * (1 - y.to(F64)))[:, 0]
    judge(rec, 'heatmap_head_bwd', what + 'bwd', dl[..., 0], want_d, base.heatmap_head_bwd(dy, y, dtype, cpad)[..., 0])


# ------------------------------------------------------------------------------------------------ the heat-map losses
LOSS_HW = (1, 3, 35, 1023, 1025, 9216)     # scalar path only; odd bases (unaligned maps); either side of one 1024-element turn
LOSS_BT = ((1, 1), (3, 5), (2, 300))       # (2, 300): the t += 256 turn of the clip reduction


def validity_pattern(B, T, seed):
    """B == 3: a clip with no valid frame, one with exactly one, one with several; B == 2: exactly two valid frames / many."""
    v = uni((B, T), seed) < 0.7
    if B == 3:
        v[0] = False
        v[1] = False
        v[1, T // 2] = True
        v[2, :2] = True
    elif B == 2:
        v[0] = False
        v[0, 1] = True
        v[0, T - 1] = True
        v[1, 0] = True
        v[1, T - 1] = True
    else:
        v[0, 0] = True
    return v


def loss_case(HW, B, T):
    s = 17 * HW + 5 * B + T
    pred = uni((B, T, HW), s).clamp(1e-6, 1 - 1e-6)
    special = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7])
    valid = validity_pattern(B, T, s + 2)
    b, t = [int(i) for i in valid.nonzero()[-1]]               # a VALID map: its head and its tail carry the special values
    m = min(HW, 4)
    pred[b, t, :m] = special[:m]
    if HW >= 8:
        pred[b, t, HW - 4:] = special.flip(0)
    if HW == 1:
        pred[0, 0, 0] = 0.0
    return pred, uni((B, T, HW), s + 1), valid


def clip_weights_f64(valid):
    v = valid.to(F64)
    n = v.sum(dim=1, keepdim=True)
    return v / (torch.where(n > 1, n, torch.ones_like(n)) * valid.shape[0])


def heatmap_loss_f64(kind, pred, gt, valid, upstream=1.0):
    """-> loss, w [B T], d pred for `upstream`: the contract of heatmap_loss.hip written out"""
    p, g = pred.to(F64), gt.to(F64)
    if kind == 0:
        per = -(g * torch.log(p).clamp_min(-100.0) + (1 - g) * torch.log1p(-p).clamp_min(-100.0))
        d = (p - g) / (p * (1 - p)).clamp_min(float(np.float32(1e-12)))     # the floor is the float 1e-12f, in ATen too
    else:
        per = (p - g) ** 2
        d = 2 * (p - g)
    w = clip_weights_f64(valid)
    HW = pred.shape[2]
    return (per.mean(dim=2) * w).sum(), w.reshape(-1), d * (w.unsqueeze(2) * (upstream / HW))


UPSTREAM = 0.37


def check_heatmap_loss(k, kind, HW, B, T, put, rec=None, base=BASE):
    what = 'heatmap_loss %s HW%d B%d T%d ' % (('bce', 'mse')[kind], HW, B, T)
    pred, gt, valid = loss_case(HW, B, T)
    want, want_w, want_d = heatmap_loss_f64(kind, pred, gt, valid, float(np.float32(UPSTREAM)))
    got, w = k.heatmap_loss_fwd(kind, put(pred), put(gt), put(valid))
    bas, bas_w = base.heatmap_loss_fwd(kind, pred, gt, valid)
    judge(rec, 'heatmap_loss_fwd', what + 'value', got.reshape(1), want.reshape(1), bas.reshape(1))
    judge(rec, 'heatmap_loss_fwd', what + 'w', w, want_w, bas_w)
    assert bool((w.cpu()[~valid.reshape(-1)] == 0).all())
    w32, up = want_w.float(), torch.tensor(UPSTREAM)
    dp = k.heatmap_loss_bwd(kind, put(pred), put(gt), put(w32), put(up))
    bas_d = base.heatmap_loss_bwd(kind, pred, gt, w32, up)
    live = (want_d != 0).reshape(-1)
    assert bool((dp.cpu().reshape(-1)[~live] == 0).all()), what + 'gradient where there is none'
    if bool(live.any()):                   # every factor is a product or a quotient: the error is relative, element by element
        judge_rows(rec, 'heatmap_loss_bwd', what + 'bwd (elementwise)', dp.reshape(-1)[put(live)], want_d.reshape(-1)[live],
                   bas_d.reshape(-1)[live], want_d.reshape(-1)[live].abs())


# ------------------------------------------------------------------------------------------------ vector terms / eye losses
VEC_KIND_D = [('mse', 1), ('mse', 2), ('mse', 3), ('euclidean', 1), ('euclidean', 2), ('euclidean', 3), ('l1', 1), ('l1', 2),
              ('l1', 3), ('angular', 2)]                       # every (kind, D) eve_vector_terms accepts
VEC_BT = ((1, 1), (5, 65), (3, 300), (4096, 1))
MIN_ANGLE = 0.5                                                # degrees between an ordinary prediction and its target
DEGENERATE_MAX = math.degrees(math.acos(1 - 4 * EPS))          # an identical pair may read this many degrees in float32


def gaze_vec(a):
    cp = torch.cos(a[..., 0])
    return torch.stack([cp * torch.sin(a[..., 1]), torch.sin(a[..., 0]), cp * torch.cos(a[..., 1])], dim=-1)


def angle_deg_f64(p, q):
    a, b = gaze_vec(p.to(F64)), gaze_vec(q.to(F64))
    return torch.acos(((a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).clamp(-1, 1)) * DEG


def term_f64(kind, pred, tgt, valid):
    """One validity-masked term written out from losses.hip's header -> value, d value / d pred (pred's shape), w [B, T]."""
    B, T = valid.shape
    p = pred.to(F64).reshape(B, T, -1).clone().requires_grad_(True)
    q = tgt.to(F64).reshape(B, T, -1)
    if kind == 'mse':
        per = ((p - q) ** 2).mean(dim=2)
    elif kind == 'euclidean':
        per = ((p - q) ** 2).sum(dim=2).sqrt()
    elif kind == 'l1':
        per = (p - q).abs().mean(dim=2)                        # autograd of abs: sign, 0 at 0
    else:
        a, b = gaze_vec(p), gaze_vec(q)
        c = (a * b).sum(-1) / (a.norm(dim=-1).clamp_min(1e-8) * b.norm(dim=-1).clamp_min(1e-8))
        inside = (c.detach() > -1.0) & (c.detach() < 1.0)      # the clamp limit 1 - 1e-8 is 1.0 in float32
        per = torch.acos(torch.where(inside, c, c.detach().clamp(-1.0, 1.0))) * DEG    # active clamp: no gradient
    w = clip_weights_f64(valid)
    val = (per * w).sum()
    return val.detach(), torch.autograd.grad(val, p)[0].reshape(pred.shape), w


def angular_row_scale(pred, tgt, w):
    """What one float32 spacing of the cosine does to a row of the angular gradient.  The gradient is -DEG w / sin(theta) x
    dc/d(pitch, yaw) with |dc/d.| <= sin(theta); its factor 1 / sqrt(1 - c^2) has the derivative c / sin^3(theta), so an error
    delta in c -- a few spacings of 2^-24 however the cosine is computed -- moves the row by delta DEG w / sin^2(theta): 1 500
    times further at 1.5 degrees than at 90.  Rows are therefore compared in units of that sensitivity (the error reads as
    the cosine's), exactly as gaze_to_pog's rows are in units of their own Jacobian.  -> [B T]"""
    th = torch.deg2rad(angle_deg_f64(pred, tgt)).reshape(-1)
    w = w.reshape(-1)
    return torch.where(w > 0, DEG * w / torch.sin(th) ** 2, torch.ones_like(w))      # (no weight: the gradient is exactly 0)


def vec_item(kind, D, B, T, seed, flat=False):
    scale = 0.4 if kind == 'angular' else 30.0
    shape = (B, T) if (D == 1 and flat) else (B, T, D)
    pred, tgt = rnd(shape, seed, scale), rnd(shape, seed + 1, scale)
    if kind == 'angular':                                      # ordinary rows stay MIN_ANGLE apart (the host test holds it)
        close = angle_deg_f64(pred, tgt) < 2 * MIN_ANGLE
        pred[close] = pred[close] + 0.1
    valid = validity_pattern(B, T, seed + 2) if B <= 3 else uni((B, T), seed + 2) < 0.7
    if B == 5:
        valid[0] = False
        valid[1] = False
        valid[1, 64] = True                                    # one valid step, past the first wave's 64 lanes
        valid[2] = False
        valid[2, 0] = True
        valid[2, 64] = True
    if kind == 'l1' and B * T > 4:
        b, t = [int(i) for i in valid.nonzero()[-1]]
        pred[b, t] = tgt[b, t]                                 # a VALID step without a difference: sign(0) = 0
    return kind, pred, tgt, valid


def vec_items(B, T, n):
    """n terms cycling through VEC_KIND_D (D == 1 alternately as [B, T] and [B, T, 1]); every fourth differentiable term does
    NOT want its gradient."""
    items, want_grad = [], []
    for i in range(n):
        kind, D = VEC_KIND_D[i % len(VEC_KIND_D)]
        items.append(vec_item(kind, D, B, T, 100 * i + B + T, flat=(i // len(VEC_KIND_D)) % 2 == 0))
        want_grad.append(kind != 'euclidean' and i % 4 != 2)
    return items, want_grad


def degenerate_item(B, T):
    """Designated rows, judged on their own: every target is its prediction (even t) or its antipode (odd t); all valid."""
    pred = rnd((B, T, 2), 555, 0.4)
    tgt = pred.clone()
    tgt[:, 1::2, 0] = -pred[:, 1::2, 0]
    tgt[:, 1::2, 1] = pred[:, 1::2, 1] + math.pi
    return 'angular', pred, tgt, torch.ones((B, T), dtype=torch.bool)


def check_degenerate(what, value, grad, B, T):
    """value: the term; grad [B, T, 2].  Identical rows read at most DEGENERATE_MAX, antiparallel ones at least 180 - that; the
    gradient is finite and no larger than one radian per radian: 57.3 x the row's weight."""
    den = T if T > 1 else 1
    w = 1.0 / (den * B)                                        # every step is valid
    want = 180.0 * (T // 2) / den
    slack = DEGENERATE_MAX * T / den + 16 * EPS * max(want, 1.0)
    assert abs(float(value) - want) <= slack, '%s: %.6f, identical / antiparallel rows give %.6f' % (what, float(value), want)
    g = grad.detach().cpu()
    assert bool(torch.isfinite(g).all()), what + ': gradient not finite'
    assert float(g.abs().max()) <= 57.3 * w, '%s: |gradient| %.3e above 57.3 x weight %.3e' % (what, float(g.abs().max()), w)


def check_vector_terms(k, B, T, n, put, rec=None, base=BASE):
    """n ordinary terms plus one of designated rows in one vector_terms call (the wrapper splits above 32)."""
    items, want_grad = vec_items(B, T, n - 1)
    items.append(degenerate_item(B, T))
    want_grad.append(True)
    what = 'vector_terms B%d T%d n%d ' % (B, T, n)
    mv = lambda it, f: (it[0], f(it[1]), f(it[2]), f(it[3]))
    out, dps = k.vector_terms([mv(it, put) for it in items], want_grad)
    b_out, b_dps = base.vector_terms(items[:-1], want_grad[:-1])
    assert tuple(out.shape) == (n,) and len(dps) == n
    for i, (it, wg) in enumerate(zip(items[:-1], want_grad[:-1])):
        kind, D = VEC_KIND_D[i % len(VEC_KIND_D)]
        val, grad, w = term_f64(*it)
        tag = '%s D%d' % (kind, D)
        # (B > 256: the restatement's value is the ordered float32 sum of its clip means, see Restatement.vector_terms)
        judge(rec, 'vector_terms value', what + '#%d %s value' % (i, tag), out[i:i + 1], val.reshape(1), b_out[i:i + 1])
        assert (dps[i] is not None) == wg, what + '#%d: gradient wanted %s' % (i, wg)
        if wg:
            assert bool((dps[i].cpu()[~it[3]] == 0).all()), what + '#%d: gradient at an invalid step' % i
            if kind == 'angular':
                judge_rows(rec, 'vector_terms gradient', what + '#%d %s gradient (rows, in the cosine\'s units)' % (i, tag), dps[i].reshape(-1, 2),
                           grad.reshape(-1, 2), b_dps[i].reshape(-1, 2), angular_row_scale(it[1], it[2], w))
            else:
                judge(rec, 'vector_terms gradient', what + '#%d %s gradient' % (i, tag), dps[i], grad, b_dps[i])
    check_degenerate(what + 'designated rows', out[n - 1], dps[n - 1], B, T)


EYE_BT = ((1, 1), (3, 5), (2, 64), (2, 65), (1, 256))          # (2, 65): a second slot per thread; (1, 256): all four
C_ANG, C_L1 = 1.0, 0.25


def eye_case(B, T, degenerate=False):
    s = 31 * B + T
    side = []
    for i in range(2):
        it = degenerate_item(B, T) if degenerate else vec_item('angular', 2, B, T, s + 10 * i)
        pp, pt = uni((B, T), s + 10 * i + 5) * 4, uni((B, T), s + 10 * i + 6) * 4
        pv = validity_pattern(B, T, s + 10 * i + 7)
        if B * T > 2:
            b, t = [int(j) for j in pv.nonzero()[-1]]
            pp[b, t] = pt[b, t]
        side.append((it[1], it[2], it[3], pp, pt, pv))
    if not degenerate and T >= 5:                              # designated rows inside an ordinary case: INVALID, gradient exactly 0
        side[0][0][:, 3] = side[0][1][:, 3]
        side[0][2][:, 3] = False
    return side


def run_eye(k, side, mv):
    a = lambda j: tuple(mv(side[i][j]) for i in range(2))
    return k.eye_losses(a(0), a(1), a(2), a(3), a(4), a(5), C_ANG, C_L1)


def eye_f64(side):
    terms, dg, dp = [], [], []
    for s in side:
        va, ga, _ = term_f64('angular', s[0], s[1], s[2])
        vl, gl, _ = term_f64('l1', s[3], s[4], s[5])
        terms += [va, vl]
        dg.append(ga); dp.append(gl)
    return torch.stack(terms + [C_ANG * (terms[0] + terms[2]) + C_L1 * (terms[1] + terms[3])]), dg, dp


def check_eye_losses(k, B, T, put, rec=None, base=BASE):
    what = 'eye_losses B%d T%d ' % (B, T)
    side = eye_case(B, T)
    terms, dg, dp = run_eye(k, side, put)
    b_terms, b_dg, b_dp = run_eye(base, side, HERE)
    w_terms, w_dg, w_dp = eye_f64(side)
    for i, nm in enumerate(('ang_l', 'l1_l', 'ang_r', 'l1_r', 'full')):
        judge(rec, 'eye_losses terms', what + nm, terms[i:i + 1], w_terms[i:i + 1], b_terms[i:i + 1])
    for i, s in enumerate(side):
        assert bool((dg[i].cpu()[~s[2]] == 0).all()) and bool((dp[i].cpu()[~s[5]] == 0).all()), what + 'gradient at an invalid step'
        judge_rows(rec, 'eye_losses gradients', what + 'dg %s (rows, in the cosine\'s units)' % 'lr'[i], dg[i].reshape(-1, 2), w_dg[i].reshape(-1, 2),
                   b_dg[i].reshape(-1, 2), angular_row_scale(s[0], s[1], clip_weights_f64(s[2])))
        judge(rec, 'eye_losses gradients', what + 'dp %s' % 'lr'[i], dp[i], w_dp[i], b_dp[i], scale=max(float(w_dp[i].abs().max()), 1e-30))
    side = eye_case(B, T, degenerate=True)
    terms, dg, dp = run_eye(k, side, put)
    for i in range(2):
        check_degenerate(what + 'designated rows %s' % 'lr'[i], terms[2 * i], dg[i], B, T)


def check_eye_losses_refusal(k, put):
    """T = 257 does not fit a thread's four slots: refused by the argument check, before any launch."""
    import pytest
    with pytest.raises(RuntimeError, match='T <= 256'):
        run_eye(k, eye_case(1, 257), put)


# ------------------------------------------------------------------------------------------------ sumsq / Adam
ADAM_N = (1, 3, 4, 5, 1023, 100003, 2100003)    # no float4 at all; one float4 (+ tail); > 524 288 and > 1 048 576: grid-stride turns
GRAD_SCALES = (3.0, 0.01, 1.0, 30.0, 0.3)       # both sides of the clip at max_norm 5 (for the n up to 5: 0.01 and 0.3 below it)
LRS = (0.016, 0.012, 0.02, 0.001, 0.008)
BETA1, BETA2, ADAM_EPS, MAX_NORM = 0.9, 0.999, 1e-8, 5.0


def f32(x):
    return float(np.float32(x))


def sumsq_chain(n):
    """The longest chain of float32 additions an element of g passes through in eve_sumsq (optim.hip), for this n.
    sumsq_partial_kernel: b = min(1024, max(1, ceil(floor(n / 4) / 256))) workgroups of 256 threads; a thread adds the four
    squares of a float4 (3 additions), adds that to its running sum once per grid-stride turn (thread 0 takes the most turns),
    then once more for a tail element (n mod 4 of them, taken by threads 0.. of workgroup 0); the wave sum is 6 shuffle-adds,
    the four waves (s0 + s1) + (s2 + s3) are 2.  sumsq_final_kernel: a thread adds ceil(b / 256) partials, then 6 + 2 again,
    and out[0] += is the last one."""
    nvec = n // 4
    blocks = min(1024, max(1, -(-nvec // 256)))
    turns = -(-nvec // (blocks * 256))
    partial = (3 if nvec else 0) + turns + (1 if n % 4 else 0) + 6 + 2
    final = -(-blocks // 256) + 6 + 2 + 1
    return partial + final


def check_sumsq(k, n, put, rec=None, base=None):
    """The derived bound (no restatement enters: `base` is unused), bit-equality over five runs, exact accumulation onto a
    non-zero start.  What the bound can see shrinks with n: (chain + 1) x 2^-24 x sum g^2 is about one element's share of the
    sum at n = 100 003 / 24 and exceeds it beyond; at n = 2 100 003 a single dropped tail element (1 / 2 100 003 of the sum
    against a bound of 29 x 2^-24 = 1 / 578 525) would pass, so that case covers the grid-stride turns -- a lost TURN is a third of
    the sum -- and the tail elements are covered by n = 1, 3, 5, 1023 and 100 003."""
    g = rnd((n,), 42 + n, 3.0)
    dg = put(g)
    exact = float((g.to(F64) ** 2).sum())
    chain = sumsq_chain(n)
    bound = (chain + 1) * EPS * exact                          # + 1: the product itself
    runs = [k.sumsq(dg, put(torch.zeros(1))).cpu() for _ in range(5)]
    assert all(torch.equal(r, runs[0]) for r in runs), 'sumsq n%d: not bit-reproducible' % n
    err = abs(float(runs[0].to(F64)) - exact)
    print('%-58s err %.3e  bound %.3e (%d additions + 1)  ratio %.2f' % ('sumsq n%d' % n, err, bound, chain, err / bound))
    if rec is not None:
        rec['sumsq err / bound'] = max(rec.get('sumsq err / bound', 0.0), err / bound)
    assert err <= bound, 'sumsq n%d: off by %.3e, bound %.3e' % (n, err, bound)
    start = torch.tensor([f32(0.37 * exact)])
    assert torch.equal(k.sumsq(dg, put(start.clone())).cpu(), start + runs[0]), 'sumsq n%d: out is not accumulated onto its start' % n


class GuardBook(object):
    """eve_adam_guard's bookkeeping in plain Python: step, skipped_total, skipped_run, good_run, loss_scale."""

    def __init__(self, step=0, loss_scale=1.0, good_run=0):
        self.step, self.skipped_total, self.skipped_run, self.good_run, self.loss_scale = step, 0, 0, good_run, float(loss_scale)

    def skip(self):
        self.skipped_total += 1
        self.skipped_run += 1
        self.good_run = 0
        if self.skipped_run >= 2:
            self.loss_scale = max(self.loss_scale * 0.5, 1.0)
            self.skipped_run = 0

    def take(self, check_finite):
        self.step += 1
        self.skipped_run = 0
        self.good_run += 1
        if check_finite and self.good_run >= 2000:
            self.loss_scale = min(self.loss_scale * 2.0, 65536.0)
            self.good_run = 0

    def words(self):
        return [self.step, self.skipped_total, self.skipped_run, self.good_run]


def assert_guard(guard, book, what):
    g = guard.cpu()
    assert g[:4].tolist() == book.words() and float(g.view(torch.float32)[4]) == book.loss_scale, \
        '%s: guard %s scale %s, want %s scale %s' % (what, g[:4].tolist(), float(g.view(torch.float32)[4]), book.words(), book.loss_scale)


class Adam64(object):
    """clip_grad_norm_ + torch.optim.Adam on float64 copies, the moments and the step counter preloaded."""

    def __init__(self, p, m, v, step0, wd):
        self.p = torch.nn.Parameter(p.to(F64).clone())
        self.opt = torch.optim.Adam([self.p], lr=1.0, betas=(f32(BETA1), f32(BETA2)), eps=f32(ADAM_EPS), weight_decay=f32(wd))
        self.opt.state[self.p] = dict(step=torch.tensor(float(step0)), exp_avg=m.to(F64).clone(), exp_avg_sq=v.to(F64).clone())

    def step(self, g, lr, gscale=1.0):
        self.p.grad = g.to(F64) * gscale
        torch.nn.utils.clip_grad_norm_([self.p], MAX_NORM)
        self.opt.param_groups[0]['lr'] = f32(lr)
        self.opt.step()

    def tensors(self):
        st = self.opt.state[self.p]
        return self.p.detach(), st['exp_avg'], st['exp_avg_sq']


def adam_case(n):
    return rnd((n,), 41 + n), 0.1 * rnd((n,), 43 + n), rnd((n,), 44 + n).abs(), [rnd((n,), 50 + n + i, s) for i, s in enumerate(GRAD_SCALES)]


def run_adam(k, n, wd, step0, mode, mv, check=None, grads=None):
    """Five steps -> (p, m, v) on the CPU.  mode 'host': the step counter passed by the host; 'guard': the device-resident guard
    and lr_dev (rewritten between steps; the lr ARGUMENT is then a value that must not be used).  check(i, guard): after a step."""
    p0, m0, v0, gs = adam_case(n)
    gs = gs if grads is None else grads
    p, m, v = mv(p0.clone()), mv(m0.clone()), mv(v0.clone())
    guard = k.new_adam_guard(p.device, loss_scale=1.0, step=step0) if mode == 'guard' else None
    lr_dev = mv(torch.zeros(1)) if mode == 'guard' else None
    for i, g in enumerate(gs):
        dg = mv(g)
        ss = k.sumsq(dg, mv(torch.zeros(1)))
        if mode == 'guard':
            lr_dev.fill_(LRS[i])
            k.adam_step(p, dg, m, v, ss, MAX_NORM, 1.0, 123.0, BETA1, BETA2, ADAM_EPS, wd, 0, guard=guard, lr_dev=lr_dev)
            if check is not None:
                check(i, guard)
        else:
            k.adam_step(p, dg, m, v, ss, MAX_NORM, 1.0, LRS[i], BETA1, BETA2, ADAM_EPS, wd, step0 + i + 1)
    return [t.detach().cpu() for t in (p, m, v)]


@functools.lru_cache(maxsize=None)
def adam_reference(n, wd, step0):
    p0, m0, v0, gs = adam_case(n)
    ref = Adam64(p0, m0, v0, step0, wd)
    for i, g in enumerate(gs):
        ref.step(g, LRS[i])
    return ref.tensors(), [run_adam(BASE, n, wd, step0, mode, HERE) for mode in ('host', 'guard')]


def check_adam(k, n, wd, step0, put, rec=None, base=None):
    """Host-stepped and guard + lr_dev, each against float64 and against each other; the guard's words after every step."""
    want, bases = adam_reference(n, wd, step0)
    if base is not None:
        bases = [run_adam(base, n, wd, step0, mode, HERE) for mode in ('host', 'guard')]
    book = GuardBook(step=step0)

    def words(i, guard):
        book.take(False)
        assert_guard(guard, book, 'adam n%d step %d' % (n, i))
        assert float(guard.cpu().view(torch.float32)[5]) == 1.0
    got = [run_adam(k, n, wd, step0, 'host', put), run_adam(k, n, wd, step0, 'guard', put, check=words)]
    for mode, g, b in zip(('host', 'guard'), got, bases):
        for nm, a, w, bb in zip('pmv', g, want, b):
            judge(rec, 'adam ' + nm, 'adam n%d wd %g step0 %d %s %s' % (n, wd, step0, mode, nm), a, w, bb)
    for nm, a, b, w, bb in zip('pmv', got[0], got[1], want, bases[0]):
        yard = max(float((bb.to(F64) - w).abs().max()), EPS * float(w.abs().max()))
        d = float((a.to(F64) - b.to(F64)).abs().max())
        assert d <= MARGIN * yard, 'adam n%d %s: host-stepped and guarded differ by %.3e (yardstick %.3e)' % (n, nm, d, yard)


def check_loss_scale_policy(k, put):
    """good_run preset to 1999: the 2000th good step doubles the scale; at 65 536 it stays; two skips halve it, never below 1.
    The weights follow the float64 optimiser on the UNscaled gradients (the buffer holds loss_scale x the gradient)."""
    n = 5
    p0, m0, v0, gs = adam_case(n)
    for ls, grown in ((8.0, 16.0), (65536.0, 65536.0), (40000.0, 65536.0)):
        p, m, v = put(p0.clone()), put(m0.clone()), put(v0.clone())
        guard = k.new_adam_guard(p.device, loss_scale=ls, step=7)
        guard[3] = 1999
        book = GuardBook(step=7, loss_scale=ls, good_run=1999)
        g = gs[2] * ls
        k.adam_step(p, put(g), m, v, k.sumsq(put(g), put(torch.zeros(1))), MAX_NORM, 1.0, LRS[0], BETA1, BETA2, ADAM_EPS, 0.005, 0,
                    guard=guard, check_finite=True)
        book.take(True)
        assert book.loss_scale == grown and book.good_run == 0
        assert_guard(guard, book, 'loss scale %g after 2000 good steps' % ls)
        ref = Adam64(p0, m0, v0, 7, 0.005)
        ref.step(gs[2], LRS[0])
        bp, bm, bv = p0.clone(), m0.clone(), v0.clone()
        BASE.adam_step(bp, g, bm, bv, BASE.sumsq(g, torch.zeros(1)), MAX_NORM, 1.0, LRS[0], BETA1, BETA2, ADAM_EPS, 0.005, 0,
                       guard=BASE.new_adam_guard('cpu', loss_scale=ls, step=7), check_finite=True)
        judge(None, 'adam p', 'adam under loss scale %g p' % ls, p, ref.tensors()[0], bp)
    for ls, halved in ((1.0, 1.0), (1.5, 1.0), (4.0, 2.0)):
        p, m, v = put(p0.clone()), put(m0.clone()), put(v0.clone())
        guard = k.new_adam_guard(p.device, loss_scale=ls, step=7)
        book = GuardBook(step=7, loss_scale=ls)
        for _ in range(2):
            k.adam_step(p, put(gs[0]), m, v, put(torch.full((1,), float('inf'))), MAX_NORM, 1.0, LRS[0], BETA1, BETA2, ADAM_EPS, 0.005, 0,
                        guard=guard, check_finite=True)
            book.skip()
            assert_guard(guard, book, 'loss scale %g after a skipped step' % ls)
        assert book.loss_scale == halved
        assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0) and torch.equal(v.cpu(), v0), 'a skipped step touched the weights'


# ------------------------------------------------------------------------------------------------ the autograd shells
SHELLS = ('GazeToPoGFn', 'MakeHeatmapsFn', 'SoftArgmaxFn', 'HeatmapHeadFn', 'HeatmapLossFn', 'VectorTermsFn', 'EyeLossesFn')
SHELL_N, SHELL_HW = 37, (5, 7)


def _shell_operands():
    f = frames(SHELL_N)
    c, _, _ = heat_case(5, 7, SHELL_N)
    heat, _ = soft_maps(5, 7, SHELL_N)
    pred, gt, valid = loss_case(35, 3, 5)
    items, _ = vec_items(3, 5, 10)
    return dict(f=f, up_mm=rnd((2, SHELL_N), 201), up_px=rnd((2, SHELL_N), 202), c=c, up_map=rnd((SHELL_N, 1, 7, 5), 203), heat=heat,
                up_x=rnd((SHELL_N,), 204), logits=rnd((2, 5, 7, 4), 205, 3.0), up_y=rnd((2, 1, 7, 5), 206), pred=pred.view(3, 5, 1, 5, 7),
                gt=gt.view(3, 5, 1, 5, 7), valid=valid, items=items, vec_w=[0.0 if i % 3 == 1 else 0.5 + i for i in range(10)],
                eye=eye_case(3, 5))


def shell_gradients(name, device):
    """The input gradient(s) of one shell under the process's default kernels on `device`: the loss reads only some of the
    outputs, and the upstream gradient reaches the shell non-contiguous (a transposed weight).  -> list of CPU tensors."""
    from eve_amd import losses, ops
    o = _shell_operands()
    mv = lambda t: t.to(device)
    leaf = lambda t: t.clone().to(device).requires_grad_(True)
    if name == 'GazeToPoGFn':
        f, g = o['f'], leaf(o['f']['g'])
        _, mm, px = ops.GazeToPoGFn.apply(g, mv(f['o']), mv(f['R']), mv(f['inv']), mv(f['ppm']), SCREEN, mv(f['head_R']), mv(f['kappa']))
        ((mm * mv(o['up_mm']).t()).sum() + (px * mv(o['up_px']).t()).sum()).backward()
        return [g.grad.cpu()]
    if name == 'MakeHeatmapsFn':
        c = leaf(o['c'])
        maps = ops.MakeHeatmapsFn.apply(c, 3.0, SHELL_HW, SCREEN)
        (maps.transpose(2, 3)[:, :, ::2] * mv(o['up_map'])[:, :, ::2]).sum().backward()
        return [c.grad.cpu()]
    if name == 'SoftArgmaxFn':
        h = leaf(o['heat'])
        px = ops.SoftArgmaxFn.apply(h, SCREEN)
        (px * mv(torch.stack([o['up_x'], torch.zeros(SHELL_N)])).t()).sum().backward()      # [2, N] transposed: strided; y unused
        return [h.grad.cpu()]
    if name == 'HeatmapHeadFn':
        lg = leaf(o['logits'])
        y = ops.HeatmapHeadFn.apply(lg)
        (y.transpose(2, 3)[:, :, 1:] * mv(o['up_y'])[:, :, 1:]).sum().backward()
        return [lg.grad.cpu()]
    if name == 'HeatmapLossFn':
        p = leaf(o['pred'])
        bce = ops.HeatmapLossFn.apply(p, mv(o['gt']), mv(o['valid']), 0)
        mse = ops.HeatmapLossFn.apply(p, mv(o['gt']), mv(o['valid']), 1)
        (UPSTREAM * bce + 1.3 * mse).backward()
        return [p.grad.cpu()]
    if name == 'VectorTermsFn':
        preds = [it[1].clone().to(device).requires_grad_(it[0] != 'euclidean') for it in o['items']]
        out = ops.VectorTermsFn.apply(tuple((it[0], mv(it[2]), mv(it[3])) for it in o['items']), *preds)
        sum(w * v for w, v, p in zip(o['vec_w'], out, preds) if p.requires_grad and w).backward()
        return [p.grad.cpu() if p.grad is not None else torch.zeros(p.shape) for p in preds if p.requires_grad]
    side = o['eye']
    lv = [leaf(side[0][0]), leaf(side[1][0]), leaf(side[0][3]), leaf(side[1][3])]
    tgt = tuple(mv(t) for t in (side[0][1], side[1][1], side[0][2], side[1][2], side[0][4], side[1][4], side[0][5], side[1][5]))
    t = losses.EyeLossesFn.apply(lv[0], lv[1], lv[2], lv[3], tgt, C_ANG, C_L1)
    (0.7 * t[4] + 0.2 * t[0]).backward()
    return [x.grad.cpu() for x in lv]


@functools.lru_cache(maxsize=None)
def shell_reference(name):
    """float64 autograd of the same losses."""
    o = _shell_operands()
    if name == 'GazeToPoGFn':
        want = pog_f64(o['f'], True)
        d = [None, o['up_mm'].t().to(F64), o['up_px'].t().to(F64)]
        g = sum(torch.einsum('ni,nij->nj', d[i], want['jac'][:, 2 * i:2 * i + 2]) for i in (1, 2))
        nb = block_norms(want['jac'])
        return [g], [d[1].abs().max(dim=1).values * nb[:, 1] + d[2].abs().max(dim=1).values * nb[:, 2]]
    if name == 'MakeHeatmapsFn':
        up = torch.zeros(SHELL_N, 1, 7, 5, dtype=F64)
        up[:, :, ::2] = o['up_map'][:, :, ::2].to(F64)
        return [heat_f64(o['c'], 3.0, SHELL_HW, up.transpose(2, 3))[1]], None
    if name == 'SoftArgmaxFn':
        return [soft_f64(o['heat'], torch.stack([o['up_x'], torch.zeros(SHELL_N)], dim=1))[1]], None
    if name == 'HeatmapHeadFn':
        lg = o['logits'].to(F64).clone().requires_grad_(True)
        y = torch.sigmoid(lg[..., 0]).unsqueeze(1)
        return [torch.autograd.grad((y.transpose(2, 3)[:, :, 1:] * o['up_y'][:, :, 1:].to(F64)).sum(), lg)[0]], None
    if name == 'HeatmapLossFn':
        flat = lambda t: t.reshape(3, 5, 35)
        d = sum(heatmap_loss_f64(kind, flat(o['pred']), flat(o['gt']), o['valid'], up)[2] for kind, up in ((0, UPSTREAM), (1, 1.3)))
        return [d.reshape(o['pred'].shape)], 'elementwise'
    if name == 'VectorTermsFn':
        return [term_f64(*it)[1] * w for it, w in zip(o['items'], o['vec_w']) if it[0] != 'euclidean'], None
    side = o['eye']
    _, dg, dp = eye_f64(side)
    return [dg[0] * (0.7 * C_ANG + 0.2), dg[1] * (0.7 * C_ANG), dp[0] * (0.7 * C_L1), dp[1] * (0.7 * C_L1)], None


def shell_base(name, k=BASE):
    """The shell over the float32 restatement (or a copy of it), on the CPU; the default kernels are put back afterwards."""
    from eve_amd import kernels
    before = kernels._default
    kernels.set_default_kernels(k)
    try:
        return shell_gradients(name, 'cpu')
    finally:
        kernels.set_default_kernels(before)


def check_shell(name, device, rec=None, got=None):
    want, rows = shell_reference(name)
    got = shell_gradients(name, device) if got is None else got
    bas = shell_base(name)
    assert len(got) == len(want) == len(bas)
    for i, (a, w, b) in enumerate(zip(got, want, bas)):
        what = 'shell %s input %d' % (name, i)
        if rows == 'elementwise':
            live = (w != 0).reshape(-1)
            assert bool((a.reshape(-1)[~live] == 0).all())
            judge_rows(rec, 'shell ' + name, what, a.reshape(-1)[live], w.reshape(-1)[live], b.reshape(-1)[live], w.reshape(-1)[live].abs())
        elif rows is not None:
            judge_rows(rec, 'shell ' + name, what, a, w, b, rows[i])
        elif float(w.abs().max()) == 0:
            assert bool((a == 0).all()), what + ': a gradient where the loss has none'
        else:
            judge(rec, 'shell ' + name, what, a, w, b)


# ------------------------------------------------------------------------------------------------ the grid, shared by both suites
def _case(fn, *args):
    return ('-'.join(str(a).replace('torch.', '') for a in args) or fn.__name__, fn, args)


GRID = {
    'gaze_to_pog': [_case(check_gaze_to_pog, N, a) for N in POG_N for a in (False, True)],
    'gaze_to_pog_bwd': [_case(check_gaze_to_pog_bwd, N, a) for N in POG_N for a in (False, True)],
    'combined_gaze': [_case(check_combined_gaze, N) for N in POG_N],
    'make_heatmaps': [_case(check_make_heatmaps, H, W, N, s) for (H, W) in HEAT_HW for N in HEAT_N for s in SIGMAS],
    'soft_argmax': [_case(check_soft_argmax, H, W, N) for (H, W) in HEAT_HW for N in HEAT_N],
    'chunked_maps': [_case(check_chunked_maps)],
    'heatmap_head': [_case(check_head, *c) for c in HEAD_CASES],
    'heatmap_loss': [_case(check_heatmap_loss, kind, HW, B, T) for kind in (0, 1) for HW in LOSS_HW for (B, T) in LOSS_BT],
    'vector_terms': [_case(check_vector_terms, B, T, n) for (B, T, n) in ((1, 1, 11), (5, 65, 32), (3, 300, 33), (4096, 1, 11), (3, 5, 11))],
    'eye_losses': [_case(check_eye_losses, B, T) for (B, T) in EYE_BT],
    'sumsq': [_case(check_sumsq, n) for n in ADAM_N],
    'adam': [_case(check_adam, n, wd, 0) for n in ADAM_N for wd in (0.0, 0.005)] + [_case(check_adam, 1023, 0.005, 10000),
                                                                                   _case(check_adam, 100003, 0.0, 10000)],
}


def grid(family):
    return GRID[family]


def grid_id(case):
    return case[0]


def run_case(case, k, put, rec=None, **kw):
    _, fn, args = case
    return fn(k, *args, put, rec, **kw)
