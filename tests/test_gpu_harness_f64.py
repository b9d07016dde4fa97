"""GPU: the kernels EVE.forward and the train step run around the two networks -- eve_amd/csrc/gaze_geometry.hip,
heatmap_loss.hip, losses.hip and sumsq / Adam of optim.hip -- and their autograd shells, against float64 at the shapes where
they can go wrong (tests/harness_ref.py: references, grids, helpers; pinned and shown to bite by tests/test_harness_ref_host.py).

The rule everywhere: the error of a tensor against float64 may be at most 4 x the error of the float32 CPU restatement against
float64 on the same operands, that yardstick floored at 2^-24 of the tensor's scale.  Every case prints err, yardstick and
ratio (run with -s).  Two derived bounds stand in for it:
  * sumsq: (additions on the longest path an element takes + 1 for its square) x 2^-24 x sum g^2; harness_ref.sumsq_chain
    counts 28 additions at n = 2 100 003 and 19 at n = 1 from the kernels' launch shape.  Plus bit-equality over five runs
    and exact accumulation onto a non-zero start.
  * gaze_to_pog values, per row: 4 x 2.5e-7 (harness_ref.POG_ROW_REL, the restatement's worst row) of |mm| + |d mm / d g|, so
    that a ray grazing the screen plane loosens its own row only.

Over more than 256 clips (vector_terms at B = 4096) the restatement adds its float32 clip means in clip order, as the one
thread of vector_terms_kernel does, so the yardstick carries the rounding of a 4096-term sequential sum (17 to 29 x 2^-24 of
the value; a pairwise mean() has one or two) and the 4 x rule holds there too.  At n = 2 100 003 sumsq's bound exceeds one
element's share of the sum: that case covers the grid-stride turns, the smaller n the tail elements.

The angular gradients (vector_terms, eye_losses) are compared row by row in units of what one float32 spacing of the cosine
does to that row, DEG w / sin^2(theta) (harness_ref.angular_row_scale).  Against the tensor's maximum, a 2-degree row of a
single-step clip reads 4.32 x the restatement -- both carry three spacings of error in the cosine there, 760 times
amplified -- which says nothing about the kernel; in the cosine's units the same row reads 1.18.

Worst ratio (error against float64) / (restatement's error against float64, floored) per kernel, MI355X, all at most 4:
    gaze_to_pog g_out 2.27, Jacobians 3.29; values per row 0.29 of their bound     gaze_to_pog_bwd 3.30
    combined_gaze 2.92, its round trip 1.23
    make_heatmaps 1.04, _bwd 3.26          soft_argmax_fwd 1.93, _bwd 2.41 (own stats and float64 stats alike)
    heatmap_head fwd 1.00, bwd 1.00        heatmap_loss value / w 2.09, gradient 1.32
    vector_terms values 2.14 (1.00 at B = 4096, against the ordered sum), gradients 1.56          eye_losses terms 2.00, gradients 1.35
    adam p 1.00, m 1.24, v 1.00            sumsq 0.04 of its bound
    shells: GazeToPoGFn 1.72, MakeHeatmapsFn 1.01, SoftArgmaxFn 1.11, HeatmapHeadFn 1.00, HeatmapLossFn 0.92,
            VectorTermsFn 1.65, EyeLossesFn 0.97
x (1 / (W - 1)) is exactly 1 at the last column of every tested size: a corner spike returns the corner bit for bit.
"""
import pytest

import harness_ref as R
from test_gpu_kernels import dev, hip  # noqa: F401  (hip: the module-scoped fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ratios():
    record = {}
    yield record
    for key, r in sorted(record.items()):
        print('\nworst ratio: %-28s %.2f' % (key, r), end='')
    print()


def cases(family):
    return pytest.mark.parametrize('case', R.grid(family), ids=R.grid_id)


@cases('gaze_to_pog')
def test_gaze_to_pog_values_and_all_twelve_jacobian_entries(hip, ratios, case):
    """N = 1, either side of one 128-thread workgroup, 300; plain and with the kappa augmentation.  Values per row, the three
    2 x 2 Jacobians per row, exact zeros in the px rows of off-screen axes, the clamp value itself off-screen."""
    R.run_case(case, hip, dev, ratios)


@cases('gaze_to_pog_bwd')
def test_gaze_to_pog_backward_for_every_combination_of_upstream_gradients(hip, ratios, case):
    """All eight present / absent combinations (none: zeros) on the float64 Jacobians, then chained on the kernel's own."""
    R.run_case(case, hip, dev, ratios)


@cases('combined_gaze')
def test_combined_gaze_and_its_round_trip_through_gaze_to_pog(hip, ratios, case):
    R.run_case(case, hip, dev, ratios)


@cases('make_heatmaps')
def test_heatmaps_forward_mask_and_backward(hip, ratios, case):
    """2 x 2 up to 72 x 128 (H W < 256 leaves lanes of the block reductions idle), 1 and 37 maps, sigma 10 / 3 / 0.7; a centre
    exactly on a pixel, centres far off-screen; invalid maps exactly 0, valid ones untouched by the mask."""
    R.run_case(case, hip, dev, ratios)


@cases('soft_argmax')
def test_soft_argmax_forward_and_backward_on_both_kinds_of_stats(hip, ratios, case):
    """Flat, a spike in each corner (px IS the corner, the gradient finite), a near-saturated map, noisy Gaussians; the
    backward chained on the kernel's own stats and on stats built from float64."""
    R.run_case(case, hip, dev, ratios)


@cases('chunked_maps')
def test_the_second_chunk_of_the_two_chunked_wrappers(hip, ratios, case):
    """65 539 maps of 2 x 2: kernels.make_heatmaps and kernels.soft_argmax_bwd launch 65 535 maps at a time."""
    R.run_case(case, hip, dev, ratios)


@cases('heatmap_head')
def test_heatmap_head_in_three_formats_with_extreme_logits(hip, ratios, case):
    """Logits 0, +-20, +-90 and the format's largest finite value: finite, in [0, 1], within the rule.  Cpad 8, and 4 for
    float32; 1 and 257 pixels, and 2 x 8192 x 256 + 77 (a second grid-stride turn and a tail) as one bf16 tensor.  The
    padding channels of dlogits are exactly 0."""
    R.run_case(case, hip, dev, ratios)


@cases('heatmap_loss')
def test_heatmap_losses_on_aligned_unaligned_and_tail_paths(hip, ratios, case):
    """HW 1, 3, 35 (maps at odd offsets: the scalar path), 1023 / 1025 (either side of one turn, the `i + 3 < HW` tail), 9216;
    (B, T) up to (2, 300) (the t += 256 turn of the clip reduction); clips with 0, 1, 2 and several valid frames; pred with
    exact 0, 1, 1e-30 and 1 - 1e-7 at the head and the tail of a valid map.  Value, w, and the gradient for an upstream of
    0.37, element by element."""
    R.run_case(case, hip, dev, ratios)


@cases('vector_terms')
def test_vector_terms_every_kind_and_width(hip, ratios, case):
    """Every (kind, D) the kernel accepts, (B, T) from (1, 1) to (4096, 1) and (3, 300); 32 terms in one launch, 33 through the
    wrapper's second; terms without a wanted gradient between terms with one; a term of designated identical / antiparallel
    rows judged on its own."""
    R.run_case(case, hip, dev, ratios)


@cases('eye_losses')
def test_eye_losses_five_terms_and_four_gradients(hip, ratios, case):
    """T = 1, 5, 64, 65 (a thread's second slot), 256 (all four slots)."""
    R.run_case(case, hip, dev, ratios)


def test_eye_losses_refuses_more_than_256_steps(hip):
    R.check_eye_losses_refusal(hip, dev)


@cases('sumsq')
def test_sumsq_within_its_addition_count_reproducible_and_accumulating(hip, ratios, case):
    R.run_case(case, hip, dev, ratios)


@cases('adam')
def test_adam_five_steps_host_stepped_and_guarded_with_lr_dev(hip, ratios, case):
    """n from 1 to 2 100 003 (grid-stride turns of adam_kernel and sumsq_partial_kernel), gradient scales on both sides of the
    clip, wd 0 and 0.005, a start at step 10 000; lr_dev rewritten between steps while the lr argument holds a value that must
    not be used; the guard's words after every step."""
    R.run_case(case, hip, dev, ratios)


def test_loss_scale_growth_ceiling_and_floor(hip):
    R.check_loss_scale_policy(hip, dev)


@pytest.mark.parametrize('name', R.SHELLS)
def test_autograd_shells_against_float64_autograd(hip, ratios, name):
    """A loss over some of the outputs only, its gradient reaching the shell non-contiguous.  The shells take the process's
    default kernels: those must be the HIP ones, not a stand-in an earlier test left behind."""
    from eve_amd import kernels
    assert isinstance(kernels.default_kernels(), kernels.HipKernels)
    R.check_shell(name, 'cuda', ratios)
