"""GPU: the InstanceNorm statistics of every route against a float64 reference, on planes where a float32 statistic can go
wrong -- a mean many standard deviations away from zero, exactly constant planes (var = 0, rstd = 1/sqrt(eps)), a Gaussian
bump on a constant background, and for the one-pass shifted kernel a nearly constant plane whose sampled pixels are outliers.

The reference is computed on exactly the values the kernel reads: the stored 16-bit / float32 tensor, or for the fused stem
the float64 7x7/2 convolution of the same packed 16-bit input and filter (the kernel's float32 MFMA accumulators are that
convolution up to float32 summation).  Bounds are those of a correct float32 algorithm (two passes, or sums shifted to a
value inside the plane's spread), not of a particular kernel:
  mean       |err| <= 2e-5 |mean| + 1e-5 sigma   (a float32 sum of the plane rounds its running value to ~1e-7 relative)
  rstd       relative error <= 2e-3 up to 300 sigma (a shifted one-pass variance in float32 carries the shift's residue
             squared times ~1e-7; the plain E[x^2] - E[x]^2 loses (mean / sigma)^2 x 6e-8 and fails near 100-300 sigma);
             <= 1e-5 for the two-pass statistics kernel (its second pass sums squares of centred values)
  constant   rstd within 1e-4 of 1/sqrt(eps), outputs equal act(beta) within one unit of the format
Family (a), zero-centred noise, runs through every route too: a bound loose enough to pass anything would show there.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
HALVES = [torch.bfloat16, torch.float16]
HALF_IDS = ['bf16', 'fp16']
DTYPES = [torch.float32] + HALVES
DT_IDS = ['f32'] + HALF_IDS
# per-element tolerance of the storage format (tests/test_gpu_kernels.py close()) and its unit roundoff
TOL = {torch.float32: 3e-5, torch.bfloat16: 1.6e-2, torch.float16: 2e-3}
REL_L2 = {torch.float32: 2e-5, torch.bfloat16: 3e-3, torch.float16: 4e-4}
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


@pytest.fixture(scope='module')
def hip():
    from eve_amd.kernels import HipKernels
    assert torch.cuda.is_available(), 'GPU suite needs a GPU'
    return HipKernels()


def last(hip):
    return hip.lib.eve_last_kernel().decode()


def dev(t):
    return None if t is None else t.cuda()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(got, want, dtype, what, scale=None, slack=None):
    """tests/test_gpu_kernels.py close(): max |diff| and relative L2 at the storage format's resolution (want in float64);
    slack: a per-element allowance taken off |diff| first (see xab_slack)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, '%s: shape %s vs %s' % (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), '%s: non-finite values' % what
    s = float(want.abs().max()) if scale is None else scale
    tol = TOL[dtype] * max(s, 1e-6)
    diff = (got - want).abs() if slack is None else ((got - want).abs() - slack).clamp_min(0)
    err = float(diff.max())
    assert err <= tol, '%s: max|diff| %.3e > tol %.3e (scale %.3e)' % (what, err, tol, s)
    rel = float(diff.norm()) / max(float(want.norm()), 1e-30)
    assert rel <= REL_L2[dtype] or err <= 1e-6 * max(s, 1e-6), '%s: relative L2 %.3e' % (what, rel)


# ---------------------------------------------------------------------------------------------------- float64 reference
def ref_stats(x):
    """[N, H, W, C] (any dtype) -> float64 mean, biased var, rstd, each [N, C]."""
    xd = x.detach().double().cpu()
    mean = xd.mean(dim=(1, 2))
    var = ((xd - mean[:, None, None, :]) ** 2).mean(dim=(1, 2))
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def check_stats(mr, mean, var, rstd, rstd_bound, what, value_err=None):
    """mr [N, C, 2] float32 from the kernel against the float64 statistics; returns (max mean error, max rstd error).
    value_err [N, C]: a bound on how far the values the kernel summed may lie from the reference's (the fused stem sums its
    float32 accumulators, the reference the float64 convolution); it adds to the mean bound, and relative to sigma to rstd's."""
    mr = mr.detach().double().cpu()
    assert torch.isfinite(mr).all(), '%s: non-finite statistics' % what
    sigma = var.sqrt()
    merr = (mr[..., 0] - mean).abs()
    mtol = 2e-5 * mean.abs() + 1e-5 * sigma
    if value_err is not None:
        mtol = mtol + value_err
        rstd_bound = rstd_bound + torch.where(var > 0, value_err / sigma.clamp_min(1e-30), torch.zeros_like(var))
    bad = merr > mtol
    assert not bad.any(), '%s: mean error %.3e > %.3e at %d planes (mean %.4g, sigma %.3g)' % (
        what, float(merr[bad].max()), float(mtol[bad].min()), int(bad.sum()), float(mean[bad][0]), float(sigma[bad][0]))
    rerr = ((mr[..., 1] - rstd) / rstd).abs()
    const = var == 0
    if const.any():                                      # var = 0: rstd = 1/sqrt(eps), judged against eps itself
        cerr = float(rerr[const].max())
        assert cerr <= 1e-4, '%s: rstd of a constant plane off by %.3e (relative)' % (what, cerr)
    bound = torch.as_tensor(rstd_bound, dtype=torch.float64).expand_as(rerr)
    k = (mean.abs() / sigma.clamp_min(1e-30))
    worst = int((rerr / bound).argmax())
    assert float((rerr / bound).max()) <= 1, '%s: rstd relative error %.3e > %.2e (plane with |mean|/sigma = %.3g, sigma %.3g)' % (
        what, float(rerr.view(-1)[worst]), float(bound.reshape(-1)[worst]), float(k.view(-1)[worst]), float(sigma.view(-1)[worst]))
    return float(merr.max()), float(rerr.max())


# ---------------------------------------------------------------------------------------------------- plane families
FAMILIES = ['centred', 'k3', 'k30', 'k100', 'k300', 'constant', 'bump']


def planes(shape, dtype, family, seed=0):
    """The family's planes, built in the storage format.  Offset families alternate sigma = 1 and sigma = 0.01 over the
    channels; 'constant' holds all-zero planes (the whole first image and every fourth channel) and nonzero constants."""
    N, H, W, C = shape
    g = gen(seed)
    noise = torch.randn(shape, generator=g, dtype=torch.float64)
    sig = torch.where(torch.arange(C) % 2 == 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.01, dtype=torch.float64))
    sign = torch.where(torch.rand((N, 1, 1, C), generator=g) < 0.5, -1.0, 1.0).double()
    if family == 'centred':
        x = noise * sig
    elif family.startswith('k'):
        k = float(family[1:])
        x = sign * k * sig + noise * sig
    elif family == 'constant':
        level = sign * (0.25 + torch.rand((N, 1, 1, C), generator=g, dtype=torch.float64) * 4)
        level[:, :, :, ::4] = 0
        level[0] = 0
        x = level.expand(shape).clone()
    elif family == 'bump':                               # a heat map: exp(-r^2 / 2 s^2) on a constant background
        yy = torch.arange(H, dtype=torch.float64)[None, :, None, None]
        xx = torch.arange(W, dtype=torch.float64)[None, None, :, None]
        cy = torch.rand((N, 1, 1, C), generator=g, dtype=torch.float64) * H
        cx = torch.rand((N, 1, 1, C), generator=g, dtype=torch.float64) * W
        s = 0.5 + torch.rand((N, 1, 1, C), generator=g, dtype=torch.float64) * 2
        bg = sign * torch.rand((N, 1, 1, C), generator=g, dtype=torch.float64) * 3
        x = bg + torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    else:
        raise ValueError(family)
    return x.to(dtype)


# ---------------------------------------------------------------------------------------------------- instnorm_stats
STATS_SHAPES = [(2, 72, 128, 16), (3, 32, 32, 64), (2, 4, 4, 512), (1, 7, 5, 8)]


def stats_kernel(dtype, shape):
    N, H, W, C = shape
    if dtype != torch.float32 and H * W * C * 2 >= 65536:
        return 'in_stats1_kernel'
    return 'in_stats_kernel'


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('shape', STATS_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_instnorm_stats_against_float64(hip, shape, dtype, family):
    x = planes(shape, dtype, family, seed=1)
    mr = hip.instnorm_stats(dev(x), EPS)
    name = last(hip)
    want = stats_kernel(dtype, shape)
    assert name.startswith(want + '<'), name
    mean, var, rstd = ref_stats(x)
    check_stats(mr, mean, var, rstd, 1e-5 if want == 'in_stats_kernel' else 2e-3, '%s %s' % (name, family))


@pytest.mark.parametrize('dtype', HALVES, ids=HALF_IDS)
@pytest.mark.parametrize('shape', [(2, 72, 128, 16), (3, 32, 32, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_one_pass_statistics_with_outliers_at_the_sampled_pixels(hip, shape, dtype):
    """in_stats1_kernel shifts by the mean of `phases` pixels px = ph * HW / phases: make exactly those pixels outliers on a
    nearly constant plane, so that the shift sits as far from the plane's mean as such a plane allows."""
    N, H, W, C = shape
    HW = H * W
    phases = 256 // (C // 8)
    g = gen(3)
    x = 1.0 + 0.01 * torch.randn((N, HW, C), generator=g, dtype=torch.float64)
    px = torch.tensor([ph * HW // phases for ph in range(phases)])
    x[:, px, :] += 8.0 * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    x = x.reshape(shape).to(dtype)
    mr = hip.instnorm_stats(dev(x), EPS)
    assert last(hip).startswith('in_stats1_kernel<'), last(hip)
    mean, var, rstd = ref_stats(x)
    check_stats(mr, mean, var, rstd, 2e-3, 'in_stats1 outliers')


# ---------------------------------------------------------------------------------------------------- instnorm_fwd_fused
# shapes of tests/test_gpu_kernels.py PLANE_CASES that reach each form of the 16-bit kernel without affine parameters:
# one workgroup per plane, two channel halves (in_split: 4 097 .. 8 192 vectors), channel parts (in_big_planes)
FUSED_SHAPES = [((2, 5, 8, 64), 'one'), ((1, 7, 5, 8), 'one'), ((2, 16, 16, 128), 'one'), ((3, 32, 32, 64), 'split'),
                ((2, 18, 32, 64), 'split'), ((2, 64, 64, 64), 'big'), ((2, 72, 128, 16), 'big')]


def fused_form(shape, dtype, affine):
    """fused_plan (norm_fused.hip) in brief: the part count the kernel must run with, or None if the plane does not fit."""
    N, H, W, C = shape
    cv = C // (4 if dtype == torch.float32 else 8)
    nvec = H * W * cv
    half = dtype != torch.float32
    sl = 0
    if half and 4096 < nvec <= 8192 and cv >= 2:
        sl, nvec, cv = 1, nvec // 2, cv // 2
    if half and not affine:
        while nvec > 8192 and cv >= 2:
            sl, nvec, cv = sl + 1, nvec // 2, cv // 2
    if nvec > 8192 and not (half and not affine and nvec <= 9216):
        return None
    return sl


def xab_slack(x, rstd, gamma):
    """The InstanceNorm apply kernels form y = x * a + b, a = gamma * rstd, b = beta - mean * a, in float32: |x| a and |b| are
    each rounded at 2^-24 before they cancel -- up to 2^-23 |x| a where the plane sits far from zero or rstd is large (a
    float32 (x - mean) * a would not lose it).  Documented bound of that form, per element."""
    g = torch.ones(x.shape[-1], dtype=torch.float64) if gamma is None else gamma.double().abs()
    return 2.0 ** -23 * x.double().abs() * (rstd * g)[:, None, None, :]


def ref_in_act(x, mean, rstd, gamma, beta, res, act):
    """float64 act(gamma * (x - mean) * rstd + beta [+ res]) with the given statistics ([N, C] float64)."""
    z = (x.double() - mean[:, None, None, :]) * rstd[:, None, None, :]
    if gamma is not None:
        z = z * gamma.double() + beta.double()
    if res is not None:
        z = z + res.double()
    return torch.relu(z) if act == 1 else z


def check_constant_outputs(y, x, var, gamma, beta, res, act, dtype, what, mean_err=None):
    """On a constant plane the output is act(beta [+ res]) to within one unit of the format: exactly so when the statistics
    are given (x - mean = 0), and up to gamma * rstd * (the mean bound) when the kernel forms the mean itself (mean_err [N, C])."""
    const = (var == 0)
    if not const.any() or res is not None:
        return
    yc = y.detach().double().cpu()
    b = torch.zeros(x.shape[-1], dtype=torch.float64) if beta is None else beta.double()
    want = b.expand(x.shape[0], x.shape[-1])
    want = torch.relu(want) if act == 1 else want
    m = const[:, None, None, :].expand(x.shape)
    w = want[:, None, None, :].expand(x.shape)
    assert torch.isfinite(yc[m]).all(), '%s: non-finite output on a constant plane' % what
    err = (yc[m] - w[m]).abs()
    unit = ULP[dtype] * w[m].abs().clamp_min(2.0 ** -14)
    gm = torch.ones(x.shape[-1], dtype=torch.float64) if gamma is None else gamma.double().abs()
    # the kernels apply x * a + b with a = gamma * rstd, b = beta - mean * a: on a constant plane that is the difference of two
    # float32 products of size |x| a, rounded at 2^-24 each (a float32 (x - mean) * a would give 0; documented bound)
    xa = (x.double().abs() * (gm / math.sqrt(EPS)))[m]
    unit = unit + 2 * 2.0 ** -24 * xa
    if mean_err is not None:
        unit = unit + (mean_err / math.sqrt(EPS) * gm)[:, None, None, :].expand(x.shape)[m]
    assert bool((err <= unit).all()), '%s: constant plane output off act(beta) by %.3e' % (what, float(err.max()))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('case', FUSED_SHAPES, ids=lambda c: 'x'.join(map(str, c[0])) + '-' + c[1])
def test_fused_instnorm_forward_against_float64(hip, case, dtype, family):
    shape, form = case
    N, H, W, C = shape
    x = planes(shape, dtype, family, seed=2)
    mean, var, rstd = ref_stats(x)
    gamma = 1 + 0.2 * torch.randn(C, generator=gen(4))
    beta = 0.1 * torch.randn(C, generator=gen(5))
    res = torch.randn(shape, generator=gen(6)).to(dtype)
    ran = []
    for (g, b, r, act, mask) in ((None, None, None, 1, False), (None, None, None, 0, False), (None, None, res, 1, True),
                                 (gamma, beta, None, 1, False)):
        sl = fused_form(shape, dtype, g is not None)
        out = hip.instnorm_fwd_fused(dev(x), dev(g), dev(b), dev(r), act, eps=EPS, want_mask=mask)
        if sl is None:
            assert out is None
            continue
        name = last(hip)
        assert name.startswith('in_fwd_fused_kernel<') or name.startswith('in_fwd_trunk_kernel<'), name
        if dtype != torch.float32 and g is None:
            assert sl == {'one': 0, 'split': 1, 'big': sl if sl >= 1 else -1}[form], (form, sl)
        ran.append(name)
        y, mr = out[0], out[1]
        what = '%s %s act=%d%s%s' % (name, family, act, ' res' if r is not None else '', ' affine' if g is not None else '')
        # the two-pass forms (every route of this kernel takes a mean pass, then a centred one)
        check_stats(mr, mean, var, rstd, 2e-3, what)
        want = ref_in_act(x, mean, rstd, g, b, r, act)
        # (the kernel forms the mean itself: a mean error within the bound above moves y by up to rstd |gamma| times it)
        gm = torch.ones(C, dtype=torch.float64) if g is None else g.double().abs()
        mslack = (rstd * gm * (2e-5 * mean.abs() + 1e-5 * var.sqrt()))[:, None, None, :]
        close(y, want, dtype, what + ' y', slack=xab_slack(x, rstd, g) + mslack)
        check_constant_outputs(y, x, var, g, b, r, act, dtype, what, mean_err=2e-5 * mean.abs())
        if mask:
            vec = 16 // x.element_size()
            bits = ((y.cpu().reshape(-1, vec) > 0).to(torch.int32) << torch.arange(vec, dtype=torch.int32)).sum(1)
            assert torch.equal(out[2].cpu().to(torch.int32), bits)
    assert ran or dtype == torch.float32


def test_fused_instnorm_single_workgroup_form_of_a_split_plane(hip):
    """The channel-split shape with in_split = 0: the same planes as one 1 024-thread workgroup each."""
    shape = (2, 18, 32, 64)
    for family in ('centred', 'k300', 'constant'):
        x = planes(shape, torch.bfloat16, family, seed=7)
        mean, var, rstd = ref_stats(x)
        with hip.dispatch_override(in_split=0):
            y, mr = hip.instnorm_fwd_fused(dev(x), None, None, None, 1, eps=EPS)
            name = last(hip)
        assert name.startswith('in_fwd_trunk_kernel<eve::bf16_t') or name.startswith('in_fwd_fused_kernel<eve::bf16_t'), name
        check_stats(mr, mean, var, rstd, 2e-3, 'in_split=0 ' + family)
        close(y, ref_in_act(x, mean, rstd, None, None, None, 1), torch.bfloat16, 'in_split=0 y ' + family,
              slack=xab_slack(x, rstd, None) + (rstd * (2e-5 * mean.abs() + 1e-5 * var.sqrt()))[:, None, None, :])


# ---------------------------------------------------------------------------------------------------- conv epilogue statistics
@pytest.mark.parametrize('hdt', HALVES, ids=HALF_IDS)
@pytest.mark.parametrize('offset', [0.0, 3.0, 30.0, 100.0, 300.0], ids=lambda o: 'k%g' % o)
def test_convolution_epilogue_statistics_against_float64(hip, hdt, offset):
    """eve_conv2d_fwd_stats (conv3x3_stream_kernel epilogue, shifted sums merged as (mean, M2) pairs) against the float64
    statistics of the y it stored; the bias sets the mean at `offset` output standard deviations."""
    N, H, W, cin, cout = 8, 72, 128, 16, 32
    x = torch.randn((N, H, W, cin), generator=gen(11)).to(hdt)
    w = (torch.randn((cout, 3, 3, cin), generator=gen(12)) * (2.0 / (9 * cin)) ** 0.5).to(hdt)
    b = offset * 1.4 * torch.where(torch.arange(cout) % 2 == 0, 1.0, -1.0) + 0.1 * torch.randn(cout, generator=gen(13))
    y, mr = hip.conv2d_fwd_stats(dev(x), dev(w), dev(b), 1, 1)
    assert last(hip).startswith('conv3x3_stream_kernel<') and mr is not None, last(hip)
    mean, var, rstd = ref_stats(y)
    k = float((mean.abs() / var.sqrt()).median())
    assert k >= 0.5 * offset, 'the planes sit %.3g standard deviations off zero, not %g' % (k, offset)
    check_stats(mr, mean, var, rstd, 2e-3, 'conv epilogue k%g' % offset)


@pytest.mark.parametrize('hdt', HALVES, ids=HALF_IDS)
def test_convolution_epilogue_statistics_of_a_constant_output(hip, hdt):
    """Zero filter: the output is the bias, a constant plane per channel (zero for some channels)."""
    N, H, W, cin, cout = 8, 72, 128, 16, 32
    x = torch.randn((N, H, W, cin), generator=gen(14)).to(hdt)
    w = torch.zeros((cout, 3, 3, cin), dtype=hdt)
    b = torch.randn(cout, generator=gen(15)) * 40
    b[::4] = 0
    y, mr = hip.conv2d_fwd_stats(dev(x), dev(w), dev(b), 1, 1)
    assert last(hip).startswith('conv3x3_stream_kernel<') and mr is not None, last(hip)
    mean, var, rstd = ref_stats(y)
    assert bool((var == 0).all())
    check_stats(mr, mean, var, rstd, 2e-3, 'conv epilogue, zero filter')


# ---------------------------------------------------------------------------------------------------- fused stem
STEM_TARGETS = [0.0, 3.0, 30.0, 100.0, 300.0]
LVL = 2.0 / 255.0                                        # one uint8 level of the [-1, 1] patch normalisation


def stem_src(N, seed):
    """[N, 3, 128, 128] patches cycling through: level +0.98 with +-1 level of texture on half the pixels, level -0.98 with
    uniform +-4 levels, a constant +0.98 patch, an all-zero patch."""
    g = gen(seed)
    src = torch.zeros((N, 3, 128, 128), dtype=torch.float64)
    for n in range(N):
        kind = n % 4
        if kind == 0:
            t = (torch.randint(0, 2, (3, 128, 128), generator=g).double() * 2 - 1) * (torch.rand((3, 128, 128), generator=g) < 0.5)
            src[n] = 0.98 + LVL * t
        elif kind == 1:
            src[n] = -0.98 + LVL * torch.randint(-4, 5, (3, 128, 128), generator=g).double()
        elif kind == 2:
            src[n] = 0.98
    return src.float()


def stem_filter(hdt, seed):
    """[64, 7, 7, 8] filter: the centre tap (kh = kw = 3, never in the zero padding) carries a per-channel mix a = (1, t, t)
    whose sum against its norm sets |mean| / sigma on a textured patch to the channel's target (0 .. 300 on the +-1 patch);
    half of the channels add small zero-mean taps elsewhere (a real convolution whose border pixels stay near the interior
    ones), the others are centre-only (a constant patch gives an exactly constant plane); two spreads (sigma ~ 1 and ~ 0.01)
    and channels 60..63 all-zero."""
    g = gen(seed)
    w = torch.zeros((64, 7, 7, 8), dtype=torch.float64)
    sd_tex = LVL * math.sqrt(0.5)                        # +-1 level on half the pixels
    targets = []
    for co in range(60):
        kt = STEM_TARGETS[co % 5]
        spread = 1.0 if (co // 5) % 2 == 0 else 0.01
        others = (co // 10) % 2 == 0
        r = min(kt * sd_tex / 0.98, math.sqrt(3.0) * (1 - 1e-9))     # (1 + 2t) / sqrt(1 + 2t^2) = r
        lo, hi = -0.5, 1.0
        for _ in range(100):
            t = 0.5 * (lo + hi)
            lo, hi = (t, hi) if (1 + 2 * t) / math.sqrt(1 + 2 * t * t) < r else (lo, t)
        a = torch.tensor([1.0, t, t], dtype=torch.float64)
        a = a / (sd_tex * a.norm()) * spread
        w[co, 3, 3, :3] = a
        if others:
            o = torch.randn((7, 7, 3), generator=g, dtype=torch.float64)
            o[3, 3] = 0
            o -= o.sum() / 146
            o[3, 3] = 0
            w[co, :, :, :3] += o * (0.003 * a.norm() / o.norm())
        targets.append(kt)
    return w.to(hdt), targets


def stem_reference(xp, w):
    """float64 7x7/2 convolution of the packed input (rows 3.., columns 4..) -> [N, 64, 64, 64] NCHW."""
    x = xp[:, 3:-3, 4:-4, :3].double().permute(0, 3, 1, 2)
    return torch.nn.functional.conv2d(x, w[..., :3].double().permute(0, 3, 1, 2), None, 2, 3)


def round_to(t, dtype):
    return t.to(dtype).double()


def check_stem_forward(xp_cpu, w, y, idx, mr, sel, hdt, what):
    conv = stem_reference(xp_cpu[sel], w)                          # [n, 64, 64, 64]
    mean = conv.mean(dim=(2, 3))
    var = ((conv - mean[:, :, None, None]) ** 2).mean(dim=(2, 3))
    rstd = 1.0 / torch.sqrt(var + EPS)
    absconv = stem_reference(xp_cpu[sel].abs(), w.abs())
    # the kernel sums its float32 accumulators: each is the float64 convolution up to 8 roundings of a running sum bounded by
    # sum |w| |x| (7 filter rows of MFMAs, K = 32 products each)
    errs = check_stats(mr[sel], mean, var, rstd, 2e-3, what, value_err=8 * 2.0 ** -24 * absconv.mean(dim=(2, 3)))
    # pooled output: relu((round(max) - mean) * rstd), the window maximum taken on the raw values and stored in the format
    # first; where the float64 maximum lies within the float32 accumulation error of a rounding boundary of the format the
    # kernel may store the neighbouring value (one unit of the raw value, times rstd)
    pooled, _ = torch.nn.functional.max_pool2d(conv, 3, 2, 1, return_indices=True)
    apool = torch.nn.functional.max_pool2d(absconv, 3, 2, 1)
    acc = 64 * 2.0 ** -24 * apool + 16 * 2.0 ** -23 * pooled.abs()  # float32 summation + the four key bits of the pooling
    lo, hi = round_to(pooled - acc, hdt), round_to(pooled + acc, hdt)
    want = torch.relu((round_to(pooled, hdt) - mean[:, :, None, None]) * rstd[:, :, None, None])
    slack = (hi - lo) * rstd[:, :, None, None]
    got = y[sel].double().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all(), what
    s = float(want.abs().max())
    err = (got - want).abs() - slack
    assert float(err.max()) <= TOL[hdt] * s, '%s: pooled output off by %.3e (tol %.3e)' % (what, float(err.max()), TOL[hdt] * s)
    inner = slack == 0
    rel = float((got - want)[inner].norm()) / max(float(want[inner].norm()), 1e-30)
    assert rel <= REL_L2[hdt], '%s: pooled output relative L2 %.3e' % (what, rel)
    # arg-max: the raw value at the chosen window position is the window maximum, within the same accumulation error
    code = idx[sel].long().cpu().permute(0, 3, 1, 2)
    kh, kw = code // 3, code % 3
    oy = (torch.arange(32)[:, None] * 2 - 1 + kh).clamp(0, 63)
    ox = (torch.arange(32)[None, :] * 2 - 1 + kw).clamp(0, 63)
    assert int(code.max()) <= 8
    picked = conv.gather(2, oy.reshape(*oy.shape[:2], -1, 1).expand(-1, -1, -1, 64)).reshape(*oy.shape[:2], 32, 32, 64)
    picked = picked.gather(4, ox.unsqueeze(-1)).squeeze(-1)
    assert float(((pooled - picked) - 2 * acc).max()) <= 0, '%s: arg-max is not the window maximum' % what
    return errs, conv, mean, var, rstd


STEM_FORMS = [('pairs', {}), ('table-two-waves', dict(stem_fwd_pairs=0, stem_split=1)),
              ('table-fold', dict(stem_fwd_pairs=0, stem_split=0))]


@pytest.mark.parametrize('hdt', HALVES, ids=HALF_IDS)
@pytest.mark.parametrize('N', [3, 19, 1100])
@pytest.mark.parametrize('form', STEM_FORMS, ids=lambda f: f[0])
def test_fused_stem_statistics_against_float64(hip, form, N, hdt):
    name, override = form
    src = stem_src(N, seed=20 + N)
    w, targets = stem_filter(hdt, seed=21)
    xp = hip.stem_pack_input(dev(src), dtype=hdt)
    with hip.dispatch_override(**override):
        y, idx, mr = hip.stem_fwd_fused(xp, dev(w), eps=EPS)
        used = last(hip)
    assert used.startswith('stem_fwd_pairs_kernel<' if name == 'pairs' else 'stem_fwd_fused_kernel<'), used
    sel = list(range(min(N, 4))) + ([N - 2, N - 1] if N > 6 else [])       # (the float64 reference of a subset)
    xp_cpu = xp.cpu()
    _, conv, mean, var, rstd = check_stem_forward(xp_cpu, w, y, idx, mr.cpu(), sel, hdt, '%s N=%d' % (used, N))
    # the planes are what the filter promises: on the +-1 patch each channel's |mean| / sigma is near its target
    k = (mean[0, :60].abs() / var[0, :60].sqrt())
    for co, kt in enumerate(targets):
        assert 0.5 * kt - 1 <= float(k[co]) <= 1.5 * kt + 1, (co, kt, float(k[co]))
    assert bool((var[:, 60:] == 0).all()) and bool((var[2, 10:20] == 0).all())         # zero filters; constant patch


@pytest.mark.parametrize('hdt', HALVES, ids=HALF_IDS)
@pytest.mark.parametrize('N', [3, 19])
def test_fused_stem_backward_against_float64(hip, N, hdt):
    """stem_bwd_dx and stem_bwd_wgrad on the offset / constant planes: d(conv out) against float64 autograd of
    conv -> IN -> ReLU -> max-pool (window choice and ReLU mask: the forward's idx / y, which the backward reads), with the
    float64 statistics; the weight gradient, accumulated onto a nonzero base, against the float64 contraction of the
    packed input with the d(conv out) stem_bwd_dx stored."""
    src = stem_src(N, seed=30 + N)
    w, _ = stem_filter(hdt, seed=31)
    xp = hip.stem_pack_input(dev(src), dtype=hdt)
    y, idx, mr = hip.stem_fwd_fused(xp, dev(w), eps=EPS)
    dy = torch.randn(tuple(y.shape), generator=gen(32)).to(hdt)
    dconv = hip.stem_bwd_dx(xp, dev(w), mr, dev(dy), y, idx)
    assert last(hip).startswith('stem_bwd_dx_kernel<'), last(hip)
    xp_cpu = xp.cpu()
    x = xp_cpu[:, 3:-3, 4:-4, :3].double().permute(0, 3, 1, 2)
    conv = torch.nn.functional.conv2d(x, w[..., :3].double().permute(0, 3, 1, 2), None, 2, 3).requires_grad_(True)
    mean = conv.mean(dim=(2, 3), keepdim=True)
    var = ((conv - mean) ** 2).mean(dim=(2, 3), keepdim=True)
    z = (conv - mean) / torch.sqrt(var + EPS)
    code = idx.long().cpu().permute(0, 3, 1, 2)
    oy = (torch.arange(32)[:, None] * 2 - 1 + code // 3).clamp(0, 63)
    ox = (torch.arange(32)[None, :] * 2 - 1 + code % 3).clamp(0, 63)
    flat = (oy * 64 + ox).reshape(N, 64, -1)
    pooled = z.reshape(N, 64, -1).gather(2, flat)
    live = (y.cpu().permute(0, 3, 1, 2).reshape(N, 64, -1) > 0).double()
    (pooled * live * dy.double().permute(0, 3, 1, 2).reshape(N, 64, -1)).sum().backward()
    want = conv.grad.permute(0, 2, 3, 1)
    close(dconv, want, hdt, 'stem_bwd_dx N=%d' % N, scale=float(want.abs().max()))
    # weight gradient: onto a nonzero base, dW[co, kh, kw, c] = sum x * d(conv out); bound = the format's rounding of
    # d(conv out) (stem_bwd_wgrad recomputes it with constants that may differ in the last float bit) over sum |x| |d(conv out)|
    base = torch.randn((64, 7, 8, 4), generator=gen(33))
    dw = dev(base).clone()
    hip.stem_bwd_wgrad(xp, dev(w), mr, dev(dy), y, idx, dw)
    assert last(hip).startswith('stem_bwd_wgrad_kernel<'), last(hip)
    got = (dw.cpu().double() - base.double())[:, :, :7, :3]
    dc = dconv.cpu().double().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(x, (64, 3, 7, 7), dc, stride=2, padding=3).permute(0, 2, 3, 1)
    mag = torch.nn.grad.conv2d_weight(x.abs(), (64, 3, 7, 7), dc.abs(), stride=2, padding=3).permute(0, 2, 3, 1)
    bound = (ULP[hdt] + 1e-5) * mag + 1e-6 * float(base.abs().max())
    excess = (got - ref).abs() - bound
    assert float(excess.max()) <= 0, 'stem_bwd_wgrad N=%d: off by %.3e beyond the bound' % (N, float(excess.max()))


# ---------------------------------------------------------------------------------------------------- consumers
def ref_backward(x, mean, rstd, gamma, beta, res, act, dy, y_stored):
    """float64 autograd of y = act(gamma * IN(x) + beta [+ res]) for the given dy; the ReLU mask is the stored y's (the kernel
    reads it).  Returns dx, d res, and the per-plane sums (sum g, sum g * xhat) with g = dy * act'."""
    xd = x.double().clone().requires_grad_(True)
    N, C = x.shape[0], x.shape[-1]
    m = xd.mean(dim=(1, 2), keepdim=True)
    v = ((xd - m) ** 2).mean(dim=(1, 2), keepdim=True)
    xhat = (xd - m) / torch.sqrt(v + EPS)
    gp = torch.ones((N, C), dtype=torch.float64, requires_grad=True)
    bp = torch.zeros((N, C), dtype=torch.float64, requires_grad=True)
    z = xhat * gp[:, None, None, :] + bp[:, None, None, :]
    if gamma is not None:
        z = z * gamma.double() + beta.double()
    g = dy.double()
    if act == 1:
        g = g * (y_stored.double() > 0)
    (z * g).sum().backward()
    dx = xd.grad
    s1, s2 = bp.grad, gp.grad
    if gamma is not None:
        s1, s2 = s1 / gamma.double(), s2 / gamma.double()
    return dx, g, torch.stack([s1, s2], dim=-1)


@pytest.mark.parametrize('family', ['k3', 'k30', 'k100', 'k300', 'constant', 'bump'])
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_consumers_of_exact_statistics(hip, dtype, family):
    """instnorm_act_fwd / _bwd, instnorm_bwd_fused (with y, without y, with the sign mask) and instnorm_act2_fwd / _bwd given
    the float64 statistics rounded to float32: x * a + b and the backward sums must not lose what the statistics hold when
    the mean is far from zero or rstd is large."""
    shape = (2, 16, 16, 64)
    N, H, W, C = shape
    x = planes(shape, dtype, family, seed=40)
    mean, var, rstd = ref_stats(x)
    mr = torch.stack([mean, rstd], dim=-1).float()
    mean32, rstd32 = mr[..., 0].double(), mr[..., 1].double()
    gamma = 1 + 0.2 * torch.randn(C, generator=gen(41))
    beta = 0.1 * torch.randn(C, generator=gen(42))
    res = torch.randn(shape, generator=gen(43)).to(dtype)
    dy = torch.randn(shape, generator=gen(44)).to(dtype)
    for (g, b, r, act) in ((None, None, None, 1), (None, None, res, 1), (None, None, None, 0), (gamma, beta, None, 1)):
        what = '%s act=%d%s%s' % (family, act, ' res' if r is not None else '', ' affine' if g is not None else '')
        want = ref_in_act(x, mean32, rstd32, g, b, r, act)
        y = hip.instnorm_act_fwd(dev(x), dev(mr), dev(g), dev(b), dev(r), act)
        close(y, want, dtype, 'instnorm_act_fwd ' + what, slack=xab_slack(x, rstd32, g))
        check_constant_outputs(y, x, var, g, b, r, act, dtype, 'instnorm_act_fwd ' + what)
        y_st = want.to(dtype)
        dx_w, g_w, s_w = ref_backward(x, mean, rstd, g, b, r, act, dy, y_st)
        dscale = float(dx_w.abs().max()) + 0.05
        sscale = float(s_w.abs().max()) * 4 + 1e-3
        dx, dres, s = hip.instnorm_act_bwd(dev(dy), dev(y_st), dev(x), dev(mr), dev(g), act, r is not None)
        close(dx, dx_w, dtype, 'instnorm_act_bwd dx ' + what, scale=dscale)
        close(s, s_w, torch.float32, 'instnorm_act_bwd sums ' + what, scale=sscale)
        if r is not None:
            close(dres, g_w, dtype, 'instnorm_act_bwd dres ' + what)
        fb = hip.instnorm_bwd_fused(dev(dy), dev(y_st), dev(x), dev(mr), dev(g), act, r is not None)
        assert last(hip).startswith('in_bwd_'), last(hip)
        close(fb[0], dx_w, dtype, 'instnorm_bwd_fused dx ' + what, scale=dscale)
        close(fb[2], s_w, torch.float32, 'instnorm_bwd_fused sums ' + what, scale=sscale)
        if r is None and act == 1:                        # act' recomputed from x instead of read from y
            fx = hip.instnorm_bwd_fused(dev(dy), None, dev(x), dev(mr), dev(g), act, False, beta=dev(b))
            close(fx[0], dx_w, dtype, 'instnorm_bwd_fused dx without y ' + what, scale=dscale)
            close(fx[2], s_w, torch.float32, 'instnorm_bwd_fused sums without y ' + what, scale=sscale)
        if act == 1 and g is None:                        # ... or from the forward's sign mask
            vec = 16 // x.element_size()
            mask = ((y_st.reshape(-1, vec) > 0).to(torch.int32) << torch.arange(vec, dtype=torch.int32)).sum(1).to(torch.uint8)
            fm = hip.instnorm_bwd_fused(dev(dy), None, dev(x), dev(mr), None, act, r is not None, mask=dev(mask))
            close(fm[0], dx_w, dtype, 'instnorm_bwd_fused dx from mask ' + what, scale=dscale)
            close(fm[2], s_w, torch.float32, 'instnorm_bwd_fused sums from mask ' + what, scale=sscale)
    # two heads over the channel concatenation of two sources (RefineNet's fork), each with its own statistics
    x2 = planes((N, H, W, 32), dtype, family, seed=45)
    m2, v2, r2 = ref_stats(x2)
    mr2 = torch.stack([m2, r2], dim=-1).float()
    ctot = C + 32
    ga, ba = 1 + 0.2 * torch.randn(ctot, generator=gen(46)), 0.1 * torch.randn(ctot, generator=gen(47))
    gb, bb = 1 - 0.3 * torch.randn(ctot, generator=gen(48)), 0.2 * torch.randn(ctot, generator=gen(49))
    d_a = torch.randn((N, H, W, ctot), generator=gen(50)).to(dtype)
    d_b = torch.randn((N, H, W, ctot), generator=gen(51)).to(dtype)
    for act in (1, 0):
        y_a, y_b = hip.instnorm_act2_fwd([dev(x), dev(x2)], [dev(mr), dev(mr2)], dev(ga), dev(ba), dev(gb), dev(bb), act)
        dxs, s_a, s_b = hip.instnorm_act2_bwd(dev(d_a), dev(d_b), [dev(x), dev(x2)], [dev(mr), dev(mr2)], dev(ga), dev(ba),
                                               dev(gb), dev(bb), act)
        for head, (yh, gh, bh, dh, sh) in enumerate(((y_a, ga, ba, d_a, s_a), (y_b, gb, bb, d_b, s_b))):
            want = torch.cat([ref_in_act(x, mr[..., 0].double(), mr[..., 1].double(), gh[:C], bh[:C], None, act),
                              ref_in_act(x2, mr2[..., 0].double(), mr2[..., 1].double(), gh[C:], bh[C:], None, act)], dim=-1)
            slack = torch.cat([xab_slack(x, mr[..., 1].double(), gh[:C]), xab_slack(x2, mr2[..., 1].double(), gh[C:])], dim=-1)
            close(yh, want, dtype, 'instnorm_act2_fwd head %d %s act=%d' % (head, family, act), slack=slack)
            zc = want        # the float64 pre-activation's sign decides act' (act2_bwd recomputes it from x)
            _, _, sa = ref_backward(x, mean, rstd, gh[:C], bh[:C], None, act, dh[..., :C], zc[..., :C])
            _, _, sb = ref_backward(x2, m2, r2, gh[C:], bh[C:], None, act, dh[..., C:], zc[..., C:])
            sw = torch.cat([sa, sb], dim=1)
            close(sh, sw, torch.float32, 'instnorm_act2_bwd sums head %d %s act=%d' % (head, family, act),
                  scale=float(sw.abs().max()) * 4 + 1e-3)
        for i, (xs, ms, rs, sl) in enumerate(((x, mean, rstd, slice(0, C)), (x2, m2, r2, slice(C, ctot)))):
            ya = ref_in_act(xs, ms, rs, ga[sl], ba[sl], None, act)
            yb = ref_in_act(xs, ms, rs, gb[sl], bb[sl], None, act)
            da, _, _ = ref_backward(xs, ms, rs, ga[sl], ba[sl], None, act, d_a[..., sl], ya)
            db, _, _ = ref_backward(xs, ms, rs, gb[sl], bb[sl], None, act, d_b[..., sl], yb)
            want = da + db
            close(dxs[i], want, dtype, 'instnorm_act2_bwd dx source %d %s act=%d' % (i, family, act),
                  scale=float(want.abs().max()) + 0.05)
