"""The per-person gaze calibration of include/eve_hip.h (eve_calib_append, eve_calib_fit) in numpy float64: the contract the HIP
kernels are tested against, with the operation order, the Levenberg-Marquardt schedule and the summation order of the header.

    reduce(g, head_R, origin, R, inv_cam, ppm, target)  -> rows [N, 16], usable [N]     one eye, N frames
    pog(rows, kappa)                                     -> [N, 2] millimetres          the model the fit minimises
    fit(rows, huber_mm=None, min_samples=5)              -> dict(kappa, rms_mm, used, inliers, ok, accepted, evals)

and the scenes the tests use (make_scene): random head rotations of +-0.4 / +-0.3 rad, origins 450 .. 750 mm in front of the
screen plane, gaze +-0.35 / +-0.45 rad, targets from the model at a known kappa*, rounded to float32."""
import numpy as np

WAVE = 64
MAX_ACCEPTED = 32
MAX_EVALS = 64
KAPPA_MAX = 0.35


def _mul(A, B):
    """3 x 3 products [..., 3, 3], every entry (a0*b0 + a1*b1) + a2*b2."""
    out = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = (A[..., i, 0] * B[..., 0, j] + A[..., i, 1] * B[..., 1, j]) + A[..., i, 2] * B[..., 2, j]
    return out


def reduce(g, head_R, origin, R, inv_cam, ppm, target):
    """g [N, 2], head_R [N, 3, 3], origin [N, 3], R [N, 3, 3], inv_cam [N, 4, 4], ppm [N, 2], target [N, 2] (float32 as the kernel gets
    them) -> (rows float64 [N, 16], usable bool [N]).  Rows of unusable frames hold whatever the arithmetic gave."""
    f = lambda a, *s: np.asarray(a).astype(np.float64).reshape((-1,) + s)
    g, Rh, o, Re, T, s, c = f(g, 2), f(head_R, 3, 3), f(origin, 3), f(R, 3, 3), f(inv_cam, 4, 4), f(ppm, 2), f(target, 2)
    N = g.shape[0]
    fin = np.ones(N, dtype=bool)
    for a in (g, Rh, o, Re, T, s, c):
        fin &= np.isfinite(a.reshape(N, -1)).all(axis=1)
    with np.errstate(all='ignore'):
        p, y = g[:, 0], g[:, 1]
        cp, sp, cy, sy = np.cos(p), np.sin(p), np.cos(y), np.sin(y)
        v = np.stack([cp * sy, sp, cp * cy], axis=1)
        u = np.stack([(Rh[:, 0, j] * v[:, 0] + Rh[:, 1, j] * v[:, 1]) + Rh[:, 2, j] * v[:, 2] for j in range(3)], axis=1)
        nu = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        ux, uy, uz = u[:, 0] / nu, u[:, 1] / nu, u[:, 2] / nu
        c0 = np.sqrt(ux * ux + uz * uz)
        s0, s1, c1 = uy, ux / c0, uz / c0
        z = np.zeros(N)
        Q = np.stack([np.stack([c1, -(s1 * s0), s1 * c0], axis=1), np.stack([z, c0, s0], axis=1),
                      np.stack([-s1, -(c1 * s0), c1 * c0], axis=1)], axis=1)
        M = _mul(T[:, :3, :3], _mul(np.swapaxes(Re, 1, 2), _mul(Rh, Q)))
        rows = np.zeros((N, 16))
        rows[:, :9] = (-M).reshape(N, 9)
        for i in range(3):
            rows[:, 9 + i] = ((T[:, i, 0] * o[:, 0] + T[:, i, 1] * o[:, 1]) + T[:, i, 2] * o[:, 2]) + T[:, i, 3]
        rows[:, 12:14] = c / s
        rows[:, 14] = 1.0
        usable = fin & (c0 > 0.0) & np.isfinite(rows[:, :14]).all(axis=1) & (-rows[:, 11] / rows[:, 8] > 0.0)
    return rows, usable


def _k(kappa):
    kp, ky = float(kappa[0]), float(kappa[1])
    return np.array([np.cos(kp) * np.sin(ky), np.sin(kp), np.cos(kp) * np.cos(ky)])


def pog(rows, kappa):
    """The modelled point of gaze of every row in millimetres at the offset kappa = (pitch, yaw)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 16)
    k = _k(kappa)
    A = rows[:, :9].reshape(-1, 3, 3)
    d = (A[:, :, 0] * k[0] + A[:, :, 1] * k[1]) + A[:, :, 2] * k[2]
    ez = rows[:, 11]
    return np.stack([rows[:, 9] - ez * (d[:, 0] / d[:, 2]), rows[:, 10] - ez * (d[:, 1] / d[:, 2])], axis=1)


def ordered_sums(contrib, reverse=False):
    """contrib [n, 9] -> the 9 sums in the header's order: lane l adds rows l, l + 64, ... from 0.0, then the 64 partial sums are
    added in lane order from 0.0.  reverse: the opposite order on both levels (to measure what the order is worth)."""
    n = contrib.shape[0]
    k = max(1, -(-n // WAVE))
    c = np.zeros((k * WAVE, contrib.shape[1]))
    c[:n] = contrib
    c = c.reshape(k, WAVE, -1)
    part = np.zeros((WAVE, contrib.shape[1]))
    for j in (range(k - 1, -1, -1) if reverse else range(k)):
        part = part + c[j]
    s = np.zeros(contrib.shape[1])
    for l in (range(WAVE - 1, -1, -1) if reverse else range(WAVE)):
        s = s + part[l]
    return s


def evaluate(rows, kappa, huber_mm=None, reverse=False):
    """eval(kappa) of the header -> (S[0..8], residual lengths of the present rows)."""
    kp, ky = float(kappa[0]), float(kappa[1])
    cp, sp, cy, sy = np.cos(kp), np.sin(kp), np.cos(ky), np.sin(ky)
    k = (cp * sy, sp, cp * cy)
    a = (-(sp * sy), cp, -(sp * cy))
    b0, b2 = cp * cy, -(cp * sy)
    w = rows[:, 14]
    present = w > 0.0
    A = rows[:, :9].reshape(-1, 3, 3)
    with np.errstate(all='ignore'):
        d = [(A[:, j, 0] * k[0] + A[:, j, 1] * k[1]) + A[:, j, 2] * k[2] for j in range(3)]
        dp = [(A[:, j, 0] * a[0] + A[:, j, 1] * a[1]) + A[:, j, 2] * a[2] for j in range(3)]
        dy = [A[:, j, 0] * b0 + A[:, j, 2] * b2 for j in range(3)]
        ez, z2 = rows[:, 11], d[2] * d[2]
        rx = (rows[:, 9] - ez * (d[0] / d[2])) - rows[:, 12]
        ry = (rows[:, 10] - ez * (d[1] / d[2])) - rows[:, 13]
        Jxp = -(ez * ((dp[0] * d[2] - d[0] * dp[2]) / z2))
        Jxy = -(ez * ((dy[0] * d[2] - d[0] * dy[2]) / z2))
        Jyp = -(ez * ((dp[1] * d[2] - d[1] * dp[2]) / z2))
        Jyy = -(ez * ((dy[1] * d[2] - d[1] * dy[2]) / z2))
        r2 = rx * rx + ry * ry
        r = np.sqrt(r2)
        if huber_mm is None:
            ws, cost, inl = w, w * r2, np.ones_like(w)
        else:
            h = float(huber_mm)
            inlier = ~(r > h)
            ws = w * np.where(inlier, 1.0, h / r)
            cost = w * np.where(inlier, r2, h * ((r + r) - h))
            inl = inlier.astype(np.float64)
        contrib = np.stack([ws * (Jxp * Jxp + Jyp * Jyp), ws * (Jxp * Jxy + Jyp * Jyy), ws * (Jxy * Jxy + Jyy * Jyy),
                            ws * (Jxp * rx + Jyp * ry), ws * (Jxy * rx + Jyy * ry), cost, w * r2, inl, np.ones_like(w)], axis=1)
    contrib[~present] = 0.0
    return ordered_sums(contrib, reverse), r[present]


def _cholesky(m00, m01, m11, thr):
    with np.errstate(all='ignore'):
        ok = m00 > thr * m00
        l00 = np.sqrt(m00)
        l10 = m01 / l00
        s = m11 - l10 * l10
        ok = bool(ok and s > thr * m11)
        l11 = np.sqrt(s)
    return ok, l00, l10, l11


def fit(rows, huber_mm=None, min_samples=5, reverse=False):
    """Levenberg-Marquardt on kappa from (0, 0) over rows [n, 16] by the header's schedule.  -> dict: kappa float64 [2], rms_mm,
    used, inliers, ok, accepted, evals, residuals (the present rows' residual lengths at the solution, millimetres).  Where ok is
    False, kappa, rms_mm and inliers are 0."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 16)
    fail = lambda used, acc=0, ev=0: {'kappa': np.zeros(2), 'rms_mm': 0.0, 'used': used, 'inliers': 0, 'ok': False, 'accepted': acc,
                                      'evals': ev, 'residuals': np.zeros(0)}
    if rows.shape[0] == 0:
        return fail(0)
    kappa = np.zeros(2)
    S, res = evaluate(rows, kappa, huber_mm, reverse)
    used = int(S[8])
    if used < min_samples or used < 1 or not np.isfinite(S[5]):
        return fail(used, 0, 1)
    lam, accepted, evals, converged = 1e-3, 0, 1, False
    with np.errstate(all='ignore'):
        while not converged and evals < MAX_EVALS:
            ok, l00, l10, l11 = _cholesky(S[0] + lam * S[0], S[1], S[2] + lam * S[2], 0.0)
            if not ok:
                return fail(used, accepted, evals)
            y0 = -S[3] / l00
            y1 = (-S[4] - l10 * y0) / l11
            d1 = y1 / l11
            d0 = (y0 - l10 * d1) / l00
            finite = bool(np.isfinite(d0) and np.isfinite(d1))
            small = finite and max(abs(d0), abs(d1)) <= 1e-12
            cand = np.array([kappa[0] + d0, kappa[1] + d1])
            Sc, resc = evaluate(rows, cand, huber_mm, reverse)
            evals += 1
            if finite and Sc[5] <= S[5]:
                kappa, S, res = cand, Sc, resc
                lam = lam / 10.0
                accepted += 1
                if small:
                    converged = True
                elif accepted == MAX_ACCEPTED:
                    return fail(used, accepted, evals)
            elif small:
                converged = True
            else:
                lam = lam * 10.0
                if lam > 1e12:
                    return fail(used, accepted, evals)
    if not converged:
        return fail(used, accepted, evals)
    ok, _, _, _ = _cholesky(S[0], S[1], S[2], 1e-10)
    if not ok or np.sqrt(kappa[0] * kappa[0] + kappa[1] * kappa[1]) > KAPPA_MAX:
        return fail(used, accepted, evals)
    return {'kappa': kappa, 'rms_mm': float(np.sqrt(S[6] / S[8])), 'used': used, 'inliers': int(S[7]), 'ok': True, 'accepted': accepted,
            'evals': evals, 'residuals': res}


# ---------------------------------------------------------------------------------------------------------------- scenes
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_scene(seed, n, kappa_star, noise_mm=0.0, outliers=0, outlier_mm=(80.0, 200.0), ppm=(3.4, 3.5)):
    """n frames of one eye as float32 inputs of reduce(), with targets (pixels) from the model at kappa_star, + Gaussian noise of
    noise_mm per axis, the first `outliers` frames (after a shuffle) moved by outlier_mm[0] .. outlier_mm[1] in a random direction.
    -> dict(g, head_R, origin, R, inv_cam, ppm, target)."""
    rng = np.random.RandomState(seed)
    g = np.stack([rng.uniform(-0.35, 0.35, n), rng.uniform(-0.45, 0.45, n)], axis=1).astype(np.float32)
    head_R = np.stack([_rot(rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)) for _ in range(n)]).astype(np.float32)
    R = np.stack([_rot(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 0.0) for _ in range(n)]).astype(np.float32)
    origin = np.stack([rng.uniform(-80, 80, n), rng.uniform(-60, 60, n), rng.uniform(450, 750, n)], axis=1).astype(np.float32)
    inv_cam = np.zeros((n, 4, 4), dtype=np.float32)
    Tr = _rot(rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.0)
    inv_cam[:, :3, :3] = Tr.astype(np.float32)
    inv_cam[:, :3, 3] = np.array([260.0, 10.0, 0.0], dtype=np.float32)
    inv_cam[:, 3, 3] = 1.0
    s = np.tile(np.asarray(ppm, dtype=np.float32), (n, 1))
    rows, usable = reduce(g, head_R, origin, R, inv_cam, s, np.zeros((n, 2), dtype=np.float32))
    assert usable.all()
    mm = pog(rows, kappa_star)
    if noise_mm:
        mm = mm + rng.normal(0.0, noise_mm, mm.shape)
    if outliers:
        idx = rng.permutation(n)[:outliers]
        ang, dist = rng.uniform(0, 2 * np.pi, outliers), rng.uniform(outlier_mm[0], outlier_mm[1], outliers)
        mm[idx] += np.stack([dist * np.cos(ang), dist * np.sin(ang)], axis=1)
    target = (mm * s.astype(np.float64)).astype(np.float32)
    return {'g': g, 'head_R': head_R, 'origin': origin, 'R': R, 'inv_cam': inv_cam, 'ppm': s, 'target': target}


def scene_rows(scene):
    rows, usable = reduce(scene['g'], scene['head_R'], scene['origin'], scene['R'], scene['inv_cam'], scene['ppm'], scene['target'])
    assert usable.all()
    return rows


KAPPA_STAR = np.array([np.deg2rad(2.5), np.deg2rad(-3.0)])
HUBER_SCENE = dict(n=130, noise_mm=8.0, outliers=13, huber_mm=25.0)
