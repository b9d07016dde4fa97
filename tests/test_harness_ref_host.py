"""CPU: pins tests/harness_ref.py -- the float64 references, case grids and comparison helpers that
tests/test_gpu_harness_f64.py holds the geometry, heat-map, loss, sumsq and Adam kernels to.

  1. the float64 references equal an independent float64 statement (ATen's binary_cross_entropy under autograd, the tensor
     expressions of eve_amd/losses.py, FakeKernels.adam_step run on float64 tensors, finite differences) to 1e-12 where
     one exists;
  2. the float32 restatement passes every helper over the whole GPU grid -- its printed error against float64 is the
     yardstick the GPU error is held to;
  3. every helper FAILS on the restatement with one planted defect, so the tests are shown to bite without a wrong kernel
     ever running on a GPU;
  4. the inputs are what the checks assume: 30 % .. 70 % of the rays on-screen on each axis, no ray within 1e-2 px of a clamp
     edge, ordinary angular rows at least 0.5 degrees apart.

The denominator rule "divide by n when n > 1" and the rule "when n >= 1" are the same function: n is a count, the two differ
only at n = 1, and there the division is by 1 (test_the_n_ge_1_rule_is_the_same_function: bit for bit the same outputs).  The
rules that do differ are planted: n > 2, and "always divide by n".
"""
import pytest
import torch
import torch.nn.functional as F

import harness_ref as R
from eve_amd import losses
from harness_ref import BASE, HERE, Restatement

F64 = torch.float64
FAMILIES = sorted(R.GRID)
ALL_CASES = [(fam, c) for fam in FAMILIES for c in R.grid(fam)]


# ------------------------------------------------------------------------------------------------ 1. the references themselves
def masked_mean(per, valid):
    return losses._masked_clip_mean(per, valid)


@pytest.mark.parametrize('kind', [0, 1], ids=['bce', 'mse'])
@pytest.mark.parametrize('HW,B,T', [(3, 3, 5), (35, 2, 300), (1025, 3, 5)])
def test_the_heatmap_loss_reference_is_aten_in_float64(kind, HW, B, T):
    pred, gt, valid = R.loss_case(HW, B, T)
    want, w, d = R.heatmap_loss_f64(kind, pred, gt, valid, 0.37)
    p = pred.to(F64).clone().requires_grad_(True)
    per = F.binary_cross_entropy(p, gt.to(F64), reduction='none') if kind == 0 else (p - gt.to(F64)) ** 2
    loss = masked_mean(per.mean(dim=2), valid)
    assert abs(float(loss.detach()) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    got = torch.autograd.grad(0.37 * loss, p)[0]
    assert float(((got - d).abs() / d.abs().clamp_min(1e-300)).max()) <= 1e-12
    assert float((w.view(B, T).sum(dim=1) * B - (valid.sum(dim=1) > 0).to(F64)).abs().max()) <= 1e-12


@pytest.mark.parametrize('B,T', [(1, 1), (5, 65), (3, 300)])
def test_the_vector_term_reference_is_the_tensor_expression_in_float64(B, T):
    fns = {'mse': losses.mse_loss, 'euclidean': losses.euclidean_loss, 'l1': losses.l1_loss, 'angular': losses.angular_loss}
    items, _ = R.vec_items(B, T, 10)
    for kind, pred, tgt, valid in items:
        val, grad, _ = R.term_f64(kind, pred, tgt, valid)
        p = pred.to(F64).clone().requires_grad_(True)
        v = fns[kind](p.reshape(B, T, -1), tgt.to(F64).reshape(B, T, -1), valid)
        assert abs(float(v.detach()) - float(val)) <= 1e-12 * max(1.0, abs(float(val))), kind
        if bool(valid.any()):
            g = torch.autograd.grad(v, p)[0]
            assert float((g - grad).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max())), kind


def test_the_adam_reference_is_torch_optim_and_equals_the_written_out_update_in_float64():
    """Adam64 IS clip_grad_norm_ + torch.optim.Adam; FakeKernels.adam_step is the update written out.  On float64 tensors
    the two agree to 1e-12, host-stepped and guarded, from step 0 and from step 10 000."""
    for step0 in (0, 10000):
        for wd in (0.0, 0.005):
            n = 1023
            p0, m0, v0, gs = R.adam_case(n)
            ref = R.Adam64(p0, m0, v0, step0, wd)
            p, m, v = p0.to(F64), m0.to(F64), v0.to(F64)
            for i, g in enumerate(gs):
                ref.step(g, R.LRS[i])
                g64 = g.to(F64)
                BASE.adam_step(p, g64, m, v, (g64 ** 2).sum(), R.MAX_NORM, 1.0, R.f32(R.LRS[i]), R.f32(R.BETA1), R.f32(R.BETA2),
                               R.f32(R.ADAM_EPS), R.f32(wd), step0 + i + 1)
            for a, b in zip((p, m, v), ref.tensors()):
                assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_the_guard_book_is_the_documented_policy():
    """GuardBook against the restatement's guard over a sequence of taken and skipped steps."""
    book = R.GuardBook(step=5, loss_scale=8.0, good_run=1998)
    guard = BASE.new_adam_guard('cpu', loss_scale=8.0, step=5)
    guard[3] = 1998
    p, m, v, g = torch.ones(3), torch.zeros(3), torch.ones(3), torch.ones(3)
    for ss in (1.0, 1.0, float('inf'), 1.0, float('inf'), float('inf'), float('inf'), float('inf'), 1.0, 1.0, 1.0):
        BASE.adam_step(p, g, m, v, torch.tensor(ss), 5.0, 1.0, 0.01, 0.9, 0.999, 1e-8, 0.0, 0, guard=guard, check_finite=True)
        book.take(True) if ss < 3e38 else book.skip()
        R.assert_guard(guard, book, 'sumsq %s' % ss)
    assert book.loss_scale == 4.0 and book.skipped_total == 5 and book.step == 5 + 6      # 8 -> 16 -> 8 -> 4


def test_the_jacobian_reference_agrees_with_central_differences():
    for augment in (False, True):
        f, want = R.pog_reference(129, augment)
        h = 1e-6
        for c in range(2):
            e = torch.zeros(2, dtype=F64)
            e[c] = h
            hi, lo = R.pog_f64(f, augment, g=f['g'].to(F64) + e), R.pog_f64(f, augment, g=f['g'].to(F64) - e)
            for oi, n in enumerate(('g_out', 'mm')):
                fd = (hi[n] - lo[n]) / (2 * h)
                scale = R.block_norms(want['jac'])[:, oi]
                ok = scale < 1e4                           # a grazing ray's third derivative outruns a 1e-6 step
                err = ((fd - want['jac'][:, 2 * oi:2 * oi + 2, c]).abs().max(dim=1).values / scale)[ok]
                assert float(err.max()) <= 1e-6, (augment, n, float(err.max()))


def test_the_stats_reference_gives_the_oracles_pixels():
    """lx, ly of soft_f64's stats on the exact grid x / (W - 1) against the oracle's float32-rounded linspace: 2^-24 apart."""
    heat, dpog = R.soft_maps(17, 61, 37)
    px, _, stats = R.soft_f64(heat, dpog)
    for a in range(2):
        assert float((stats[:, a] * R.SCREEN[a] - px[:, a]).abs().max()) <= 2 * R.EPS * R.SCREEN[a]
    assert float((R.combined_reference(129)[3]['mm'] - R.combined_reference(129)[1].to(F64)).abs().max()) < 1e-3   # cam, inv are inverses


# ------------------------------------------------------------------------------------------------ 2. the restatement passes
@pytest.mark.parametrize('fam,case', ALL_CASES, ids=['%s-%s' % (f, c[0]) for f, c in ALL_CASES])
def test_the_float32_restatement_passes_every_case_of_the_gpu_grid(fam, case):
    R.run_case(case, Restatement(), HERE)


def test_the_restatement_passes_the_remaining_helpers():
    k = Restatement()
    R.check_eye_losses_refusal(k, HERE)
    R.check_loss_scale_policy(k, HERE)
    for name in R.SHELLS:
        R.check_shell(name, 'cpu', got=R.shell_base(name, k))


def test_the_per_row_bound_of_gaze_to_pog_is_the_restatements_worst_row():
    worst = max(R.pog_row_error(R.pog_base(N, a)[1], R.pog_reference(N, a)[1]) for N in R.POG_N for a in (False, True))
    print('worst row of the float32 restatement: %.3e of |mm| + |J|; recorded %.3e' % (worst, R.POG_ROW_REL))
    assert worst <= R.POG_ROW_REL <= 1.5 * worst


def test_sumsq_chain_counts():
    """The two derived counts the GPU module quotes: 28 additions at n = 2 100 003 (3 in the float4, 3 turns, 1 tail element,
    6 + 2; then 4 partials a thread, 6 + 2, and the accumulation), 19 at n = 1 (no float4: the tail element alone)."""
    assert R.sumsq_chain(2100003) == 3 + 3 + 1 + 8 + 4 + 8 + 1 == 28
    assert R.sumsq_chain(1) == 0 + 0 + 1 + 8 + 1 + 8 + 1 == 19
    assert R.sumsq_chain(100003) == 3 + 1 + 1 + 8 + 1 + 8 + 1


# ------------------------------------------------------------------------------------------------ 3. planted defects
def fails(case_or_fn, k, *args, **kw):
    with pytest.raises(AssertionError):
        if isinstance(case_or_fn, tuple):
            R.run_case(case_or_fn, k, HERE, None, **kw)
        else:
            case_or_fn(k, *args, **kw)


def pick(fam, ident):
    return [c for c in R.grid(fam) if c[0] == ident][0]


class JacobianEntryScaled(Restatement):
    def gaze_to_pog(self, *a, **kw):
        g, mm, px, jac = Restatement.gaze_to_pog(self, *a, **kw)
        jac[:, 3, 1] *= 1 + 1e-3                               # d mm_y / d yaw
        return g, mm, px, jac


class BackwardDropsAComponent(Restatement):
    def gaze_to_pog_bwd(self, jac, dg_out, dmm, dpx):
        if dpx is not None:
            dpx = dpx * torch.tensor([1.0, 0.0])
        return Restatement.gaze_to_pog_bwd(self, jac, dg_out, dmm, dpx)


class CombinedGazeYawFlipped(Restatement):
    def combined_gaze(self, *a):
        return Restatement.combined_gaze(self, *a) * torch.tensor([1.0, -1.0])


def test_a_jacobian_entry_scaled_by_a_thousandth_fails():
    for ident in ('129-False', '300-True'):
        fails(pick('gaze_to_pog', ident), JacobianEntryScaled(), base=BASE)
        fails(pick('gaze_to_pog_bwd', ident), JacobianEntryScaled(), base=BASE)          # the chained step
    fails(pick('gaze_to_pog_bwd', '128-False'), BackwardDropsAComponent(), base=BASE)
    fails(pick('combined_gaze', '127'), CombinedGazeYawFlipped(), base=BASE)
    with pytest.raises(AssertionError):
        R.check_shell('GazeToPoGFn', 'cpu', got=R.shell_base('GazeToPoGFn', BackwardDropsAComponent()))


def clip_rule(rule):
    class Rule(Restatement):
        def heatmap_loss_fwd(self, kind, pred, gt, validity):
            v = validity.float()
            n = v.sum(dim=1, keepdim=True)
            w = v / (torch.where(rule(n), n, torch.ones_like(n)) * pred.shape[0])
            per = (F.binary_cross_entropy(pred, gt, reduction='none') if kind == 0 else (pred - gt) ** 2).flatten(2).mean(dim=2)
            return (per * w).sum(), w.reshape(-1)
    return Rule()


def test_the_n_ge_1_rule_is_the_same_function():
    for case in R.grid('heatmap_loss'):
        pred, gt, valid = R.loss_case(*case[2][1:])
        a, b = clip_rule(lambda n: n > 1).heatmap_loss_fwd(case[2][0], pred, gt, valid), clip_rule(lambda n: n >= 1).heatmap_loss_fwd(case[2][0], pred, gt, valid)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        R.run_case(case, clip_rule(lambda n: n >= 1), HERE)


def test_a_changed_denominator_rule_fails():
    """n > 2 leaves the clip with exactly two valid frames undivided (B = 2 cases); "always n" divides the empty clip by 0."""
    for ident in ('0-35-2-300', '1-1-2-300', '1-9216-2-300'):
        fails(pick('heatmap_loss', ident), clip_rule(lambda n: n > 2), base=BASE)
    fails(pick('heatmap_loss', '0-3-3-5'), clip_rule(lambda n: n > -1), base=BASE)


class MapMeanDropsItsTail(Restatement):
    def heatmap_loss_fwd(self, kind, pred, gt, validity):
        loss, w = Restatement.heatmap_loss_fwd(self, kind, pred, gt, validity)
        HW = pred.shape[2]
        if HW > 1:
            p, g = pred[..., -1], gt[..., -1]
            last = F.binary_cross_entropy(p, g, reduction='none') if kind == 0 else (p - g) ** 2
            loss = loss - (last * w.view(p.shape)).sum() / HW
        return loss, w


class LossBackwardForgetsTheUpstream(Restatement):
    def heatmap_loss_bwd(self, kind, pred, gt, w, upstream):
        return Restatement.heatmap_loss_bwd(self, kind, pred, gt, w, torch.tensor(1.0))


def test_a_dropped_tail_element_in_a_map_mean_fails():
    for ident in ('0-3-3-5', '1-35-1-1', '0-1023-3-5', '1-1025-2-300', '0-9216-3-5', '1-9216-3-5'):
        fails(pick('heatmap_loss', ident), MapMeanDropsItsTail(), base=BASE)
    fails(pick('heatmap_loss', '0-35-3-5'), LossBackwardForgetsTheUpstream(), base=BASE)
    with pytest.raises(AssertionError):
        R.check_shell('HeatmapLossFn', 'cpu', got=R.shell_base('HeatmapLossFn', LossBackwardForgetsTheUpstream()))


class GridOverW(Restatement):
    """soft-argmax on the grid x / W instead of x / (W - 1)"""

    def soft_argmax_fwd(self, heat, screen):
        n, _, h, w = heat.shape
        p = F.softmax(1e2 * heat.reshape(n, h * w), dim=-1)
        xs = (torch.arange(w, dtype=torch.float32) / w).repeat(h)
        ys = (torch.arange(h, dtype=torch.float32) / (h - 1)).repeat_interleave(w)
        return torch.stack([(screen[0] * (xs * p).sum(-1)).clamp(0, screen[0]), (screen[1] * (ys * p).sum(-1)).clamp(0, screen[1])], dim=-1), \
            heat.new_zeros(n, 4)


class SoftArgmaxBackwardIgnoresY(Restatement):
    def soft_argmax_bwd(self, heat, stats, dpog, screen):
        return Restatement.soft_argmax_bwd(self, heat, stats, dpog * torch.tensor([1.0, 0.0]), screen)


def test_a_grid_over_w_instead_of_w_minus_one_fails():
    for case in R.grid('soft_argmax'):
        fails(case, GridOverW(), base=BASE)
        fails(case, SoftArgmaxBackwardIgnoresY(), base=BASE)


class SecondChunkReusesTheFirstChunksCentres(Restatement):
    def make_heatmaps(self, centres_px, sigma, hw, screen, validity=None):
        out = []
        for i in range(0, centres_px.shape[0], 65535):
            n = min(65535, centres_px.shape[0] - i)
            out.append(Restatement.make_heatmaps(self, centres_px[0:n], sigma, hw, screen, None if validity is None else validity[i:i + n]))
        return torch.cat(out)


class SecondChunkOfTheBackwardReusesTheFirstChunksGradient(Restatement):
    def soft_argmax_bwd(self, heat, stats, dpog, screen):
        out = []
        for i in range(0, heat.shape[0], 65535):
            n = min(65535, heat.shape[0] - i)
            out.append(Restatement.soft_argmax_bwd(self, heat[i:i + n], None, dpog[0:n], screen))
        return torch.cat(out)


class HeatmapCentreScaledByTheWrongAxis(Restatement):
    def make_heatmaps(self, centres_px, sigma, hw, screen, validity=None):
        c = centres_px * torch.tensor([1.0, (hw[1] / screen[0]) / (hw[0] / screen[1])])
        return Restatement.make_heatmaps(self, c, sigma, hw, screen, validity)


def test_a_second_chunk_that_reuses_the_first_chunks_rows_fails():
    fails(R.check_chunked_maps, SecondChunkReusesTheFirstChunksCentres(), HERE)
    fails(R.check_chunked_maps, SecondChunkOfTheBackwardReusesTheFirstChunksGradient(), HERE)
    SecondChunkReusesTheFirstChunksCentres().make_heatmaps(*[R.heat_case(5, 7, 37)[0], 3.0, (5, 7), R.SCREEN])
    R.run_case(pick('make_heatmaps', '5-7-37-3.0'), SecondChunkReusesTheFirstChunksCentres(), HERE)     # one chunk: no defect
    for ident in ('5-7-37-3.0', '33-31-1-0.7', '17-61-37-10.0'):           # (72 x 128 on 1080 x 1920 scales both axes alike)
        fails(pick('make_heatmaps', ident), HeatmapCentreScaledByTheWrongAxis(), base=BASE)


class BiasCorrectionOneStepBehind(Restatement):
    def adam_step(self, p, g, m, v, sumsq, max_norm, gscale, lr, beta1, beta2, eps, weight_decay, step, guard=None, **kw):
        if guard is not None:
            guard[0] -= 1
            Restatement.adam_step(self, p, g, m, v, sumsq, max_norm, gscale, lr, beta1, beta2, eps, weight_decay, step, guard=guard, **kw)
            guard[0] += 1
        else:
            Restatement.adam_step(self, p, g, m, v, sumsq, max_norm, gscale, lr, beta1, beta2, eps, weight_decay, step - 1)


class LrDevIgnored(Restatement):
    def adam_step(self, *a, **kw):
        if kw.get('lr_dev') is not None:
            kw['lr_dev'] = torch.tensor([R.LRS[0]])
        Restatement.adam_step(self, *a, **kw)


class SumsqDropsTheLastElement(Restatement):
    def sumsq(self, g, out, workspace=None):
        return Restatement.sumsq(self, g[:-1] if g.numel() > 1 else g * 0, out)


class SumsqOverwrites(Restatement):
    def sumsq(self, g, out, workspace=None):
        out.zero_()
        return Restatement.sumsq(self, g, out)


class LossScaleWithoutCeiling(Restatement):
    def adam_step(self, *a, **kw):
        guard = kw.get('guard')
        before = float(guard.view(torch.float32)[4]) if guard is not None else None
        Restatement.adam_step(self, *a, **kw)
        if guard is not None and int(guard[3]) == 0 and float(guard.view(torch.float32)[5]) == 1.0:
            guard.view(torch.float32)[4] = before * 2.0


def test_a_bias_correction_one_step_behind_fails():
    """From step 3 (at step 10 000 both corrections are 1 to a part in 10^5 and one step makes no difference that float32
    could show: that start checks powf, not this)."""
    for n, wd in ((5, 0.0), (1023, 0.005), (100003, 0.0)):
        fails(R.check_adam, BiasCorrectionOneStepBehind(), n, wd, 3, HERE)
    fails(R.check_adam, LrDevIgnored(), 1023, 0.005, 0, HERE)
    for n in (3, 5, 1023, 100003):                             # (beyond, one element is less than the derived bound: check_sumsq)
        fails(R.check_sumsq, SumsqDropsTheLastElement(), n, HERE)
    fails(R.check_sumsq, SumsqOverwrites(), 1023, HERE)
    fails(R.check_loss_scale_policy, LossScaleWithoutCeiling(), HERE)


class SigmoidInTheStorageType(Restatement):
    def heatmap_head_fwd(self, logits):
        return torch.sigmoid(logits[..., 0]).float().unsqueeze(1).contiguous()


class HeadBackwardFillsThePadding(Restatement):
    def heatmap_head_bwd(self, dy, y, dtype, cpad):
        dl = Restatement.heatmap_head_bwd(self, dy, y, dtype, cpad)
        dl[..., 1] = dl[..., 0]
        return dl


class L1NotAveragedOverD(Restatement):
    def vector_terms(self, items, want_grad):
        out, dps = Restatement.vector_terms(self, items, want_grad)
        for i, it in enumerate(items):
            if it[0] == 'l1' and it[1].dim() == 3:
                out[i] *= it[1].shape[2]
        return out, dps


class SignOfZeroIsOne(Restatement):
    def vector_terms(self, items, want_grad):
        out, dps = Restatement.vector_terms(self, items, want_grad)
        for it, d in zip(items, dps):
            if it[0] == 'l1' and d is not None:
                B, T = it[3].shape
                same = (it[1] == it[2]) & it[3].reshape([B, T] + [1] * (it[1].dim() - 2))
                d[same] = d.abs().max()
        return out, dps


class AngularGradientNotANumberAtTheClamp(Restatement):
    def vector_terms(self, items, want_grad):
        out, dps = Restatement.vector_terms(self, items, want_grad)
        for it, d in zip(items, dps):
            if it[0] == 'angular' and d is not None:
                d[(it[1] == it[2]).all(dim=-1)] = float('nan')
        return out, dps


class LastClipMeanDropped(Restatement):
    """the sum over clips stops one short (`b < B - 1`); planted in the ordered sum, the path taken above 256 clips"""

    def clip_sum(self, clip_means):
        return Restatement.clip_sum(self, clip_means[:-1])


class FullLossWithOneCoefficient(Restatement):
    def eye_losses(self, g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, coeff_ang, coeff_l1):
        return Restatement.eye_losses(self, g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, coeff_ang, coeff_ang)


class EyeLossesFourthSlotLost(Restatement):
    """t >= 192 takes the validity of t - 192"""

    def eye_losses(self, g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, coeff_ang, coeff_l1):
        if g_val[0].shape[1] > 192:
            g_val = tuple(torch.cat([v[:, :192], v[:, :v.shape[1] - 192]], dim=1) for v in g_val)
        return Restatement.eye_losses(self, g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, coeff_ang, coeff_l1)


class FakeAcceptsAnyT(Restatement):
    def eye_losses(self, g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, coeff_ang, coeff_l1):
        o, _ = self.vector_terms([('l1', p_pred[0], p_tgt[0], p_val[0])], [False])
        return o, None, None


def test_defects_in_the_head_and_the_loss_terms_fail():
    fails(pick('heatmap_head', 'bfloat16-8-257'), SigmoidInTheStorageType(), base=BASE)
    fails(pick('heatmap_head', 'float16-8-257'), SigmoidInTheStorageType(), base=BASE)
    fails(pick('heatmap_head', 'float32-4-257'), HeadBackwardFillsThePadding(), base=BASE)
    for case in R.grid('vector_terms'):
        fails(case, L1NotAveragedOverD(), base=BASE)
        fails(case, AngularGradientNotANumberAtTheClamp(), base=BASE)
    fails(pick('vector_terms', '3-300-33'), SignOfZeroIsOne(), base=BASE)
    fails(pick('vector_terms', '4096-1-11'), LastClipMeanDropped(), base=BASE)              # one clip of 4096: 2.4e-4 of the value
    for case in R.grid('eye_losses'):
        fails(case, FullLossWithOneCoefficient(), base=BASE)
    fails(pick('eye_losses', '1-256'), EyeLossesFourthSlotLost(), base=BASE)
    with pytest.raises(BaseException):
        R.check_eye_losses_refusal(FakeAcceptsAnyT(), HERE)


# ------------------------------------------------------------------------------------------------ 4. the inputs
def test_about_half_the_rays_are_on_screen_and_none_sits_on_a_clamp_edge():
    for augment in (False, True):
        for N in R.POG_N:
            _, want = R.pog_reference(N, augment)
            raw = want['raw']
            edge = torch.stack([raw[:, 0].abs(), (raw[:, 0] - R.SCREEN[0]).abs(), raw[:, 1].abs(), (raw[:, 1] - R.SCREEN[1]).abs()])
            assert float(edge.min()) >= 1e-2, (N, augment, float(edge.min()))          # no row excluded
            if N >= 127:
                share = want['on'].to(F64).mean(dim=0)
                assert bool(((share >= 0.3) & (share <= 0.7)).all()), (N, augment, share.tolist())
    _, pog, _, rt = R.combined_reference(300)
    assert bool(rt['on'].all())                                                          # the round trip stays on the screen


def test_ordinary_angular_rows_are_half_a_degree_apart():
    least, most = 180.0, 0.0
    pairs = []
    for case in R.grid('vector_terms'):
        B, T, n = case[2]
        pairs += [(it[1], it[2], it[3]) for it in R.vec_items(B, T, n - 1)[0] if it[0] == 'angular']
    for case in R.grid('eye_losses'):
        pairs += [(s[0], s[1], s[2]) for s in R.eye_case(*case[2])]
    for pred, tgt, valid in pairs:
        a = R.angle_deg_f64(pred, tgt)[valid]                  # (an eye case's designated row is invalid: judged on its own)
        if a.numel():
            least, most = min(least, float(a.min())), max(most, float(a.max()))
    print('ordinary rows: %.2f .. %.2f degrees apart' % (least, most))
    assert least >= R.MIN_ANGLE and most <= 180.0 - R.MIN_ANGLE
    _, pred, tgt, _ = R.degenerate_item(3, 8)
    a = R.angle_deg_f64(pred, tgt)
    assert float(a[:, 0::2].max()) < 1e-4 and float(a[:, 1::2].min()) > 180 - 1e-4          # yaw + pi is rounded to float32
    assert abs(R.DEGENERATE_MAX - 0.0396) < 1e-3
