"""The screen-space gaze calibration of include/eve_hip.h (eve_screen_calib_append, eve_screen_calib_fit, eve_screen_calib_apply) in
numpy float64: the contract the HIP kernels are tested against, with the header's operation order, solve schedule and summation
order (calib_ref.ordered_sums).

    reduce(pog, origin, inv_cam, ppm, target, screen_size)          -> rows [N, 12], usable [N]
    passes(rows, coef, K, huber_mm=None)                            -> the sums of one pass at the coefficients coef
    cholesky_solve(G, bx, by, K)                                    -> (ok, coef [2, 6])
    fit(rows, kind, huber_mm=None, min_samples=None, max_shift_mm)  -> dict(coef, kind, ok, used, inliers, solves, the report)
    evaluate(rows, coef, kind)                                      -> the same dict for a stored map (mode 1: nothing is solved)
    apply(px, ppm, coef, kind, screen_size)                         -> float32 [N, 2]

and the scenes the tests use (make_scene): a grid of dots on a 1920 x 1080 screen, a known map of about +-12 mm per term, the raw
points the targets pushed through its inverse, rounded to float32."""
import numpy as np

from calib_ref import _rot, ordered_sums

ROW = 12                                 # u, v, xm, ym, tmx, tmy, e0, e1, e2, the weight, two reserved 0.0
KINDS = {'offset': 1, 'affine': 2, 'quadratic': 3}
TERMS = (0, 1, 3, 6)                     # kind -> K, the terms of phi = (1, u, v, u*u, u*v, v*v) in use
MAX_SOLVES = 64
PIVOT_REL = 1e-10
STEP_TOL_MM = 1e-6
RAD2DEG = 57.29577951308232              # 180 / pi
REPORT = ('rms_mm', 'mean_mm', 'max_mm', 'mean_deg', 'rms_mm_raw', 'mean_mm_raw', 'max_mm_raw', 'mean_deg_raw')


def terms_of(kind):
    return TERMS[kind] if 0 <= kind <= 3 else 0


def reduce(pog, origin, inv_cam, ppm, target, screen_size):
    """pog [N, 2], origin [N, 3], inv_cam [N, 4, 4], ppm [N, 2], target [N, 2] (float32 as the kernel gets them), screen_size (W, H)
    -> (rows float64 [N, 12], usable bool [N]).  Rows of unusable frames hold whatever the arithmetic gave."""
    f = lambda a, *s: np.asarray(a).astype(np.float64).reshape((-1,) + s)
    p, o, T, s, c = f(pog, 2), f(origin, 3), f(inv_cam, 4, 4), f(ppm, 2), f(target, 2)
    W, H = float(screen_size[0]), float(screen_size[1])
    N = p.shape[0]
    fin = np.ones(N, dtype=bool)
    for a in (p, o, T, s, c):
        fin &= np.isfinite(a.reshape(N, -1)).all(axis=1)
    rows = np.zeros((N, ROW))
    with np.errstate(all='ignore'):
        rows[:, 0] = (p[:, 0] + p[:, 0]) / W - 1.0
        rows[:, 1] = (p[:, 1] + p[:, 1]) / H - 1.0
        rows[:, 2:4] = p / s
        rows[:, 4:6] = c / s
        for i in range(3):
            rows[:, 6 + i] = ((T[:, i, 0] * o[:, 0] + T[:, i, 1] * o[:, 1]) + T[:, i, 2] * o[:, 2]) + T[:, i, 3]
        rows[:, 9] = 1.0
        usable = fin & np.isfinite(rows).all(axis=1) & (s[:, 0] > 0.0) & (s[:, 1] > 0.0) & (rows[:, 8] != 0.0)
    return rows, usable


def phi_of(u, v):
    return [np.ones_like(u), u, v, u * u, u * v, v * v]


def shift(phi, coef, K):
    """The correction in millimetres, both axes: s_a = C[a][0]; s_a = s_a + phi_k * C[a][k], k = 1 .. K-1 (K = 0: none)."""
    out = []
    for a in range(2):
        s = np.zeros_like(phi[1])
        if K > 0:
            s = s + coef[a][0]
            for k in range(1, K):
                s = s + phi[k] * coef[a][k]
        out.append(s)
    return out


def _huber(w, r2, r, huber_mm):
    if huber_mm is None:
        return w, w * r2, np.ones_like(w)
    h = float(huber_mm)
    inlier = ~(r > h)
    return w * np.where(inlier, 1.0, h / r), w * np.where(inlier, r2, h * ((r + r) - h)), inlier.astype(np.float64)


def passes(rows, coef, K, huber_mm=None):
    """One pass at the coefficients coef [2, 6] -> dict: G [K, K] (the lower triangle filled), bx [K], by [K], cost, wr2, wr, inl, n."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    w = rows[:, 9]
    present = w > 0.0
    with np.errstate(all='ignore'):
        phi = phi_of(rows[:, 0], rows[:, 1])
        p = shift(phi, coef, K)
        ex, ey = rows[:, 4] - rows[:, 2], rows[:, 5] - rows[:, 3]
        rx, ry = p[0] - ex, p[1] - ey
        r2 = rx * rx + ry * ry
        r = np.sqrt(r2)
        ws, cost, inl = _huber(w, r2, r, huber_mm)
        cols = [ws * phi[i] * phi[j] for i in range(K) for j in range(i + 1)]
        cols += [ws * phi[i] * ex for i in range(K)] + [ws * phi[i] * ey for i in range(K)]
        cols += [cost, w * r2, w * r, inl, np.ones_like(w)]
        contrib = np.stack(cols, axis=1) if rows.shape[0] else np.zeros((0, len(cols)))
    contrib[~present] = 0.0
    S = ordered_sums(contrib)
    G = np.zeros((K, K))
    q = 0
    for i in range(K):
        for j in range(i + 1):
            G[i, j] = S[q]
            q += 1
    return {'G': G, 'bx': S[q:q + K], 'by': S[q + K:q + 2 * K], 'cost': S[q + 2 * K], 'wr2': S[q + 2 * K + 1], 'wr': S[q + 2 * K + 2],
            'inl': S[q + 2 * K + 3], 'n': S[q + 2 * K + 4]}


def cholesky_solve(G, bx, by, K):
    """G c_a = b_a for both axes by the header's row-by-row Cholesky and substitutions -> (ok, coef [2, 6]); ok False at a pivot
    that fails (G_jj > 0 and s > 1e-10 * G_jj), with the coefficients unspecified."""
    L = np.zeros((K, K))
    coef = np.zeros((2, 6))
    with np.errstate(all='ignore'):
        for j in range(K):
            s = G[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (G[j, j] > 0.0 and s > PIVOT_REL * G[j, j]):
                return False, coef
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, K):
                t = G[i, j]
                for k in range(j):
                    t = t - L[i, k] * L[j, k]
                L[i, j] = t / L[j, j]
        for a, b in enumerate((bx, by)):
            y = np.zeros(K)
            for i in range(K):
                t = b[i]
                for k in range(i):
                    t = t - L[i, k] * y[k]
                y[i] = t / L[i, i]
            for i in range(K - 1, -1, -1):
                t = y[i]
                for k in range(i + 1, K):
                    t = t - L[k, i] * coef[a][k]
                coef[a][i] = t / L[i, i]
    return True, coef


def _angle(ax, ay, bx, by, mz):
    """deg = atan2(|a x b|, a . b) * (180 / pi) with a = (ax, ay, mz), b = (bx, by, mz) and the header's brackets."""
    c0 = ay * mz - mz * by
    c1 = mz * bx - ax * mz
    c2 = ax * by - ay * bx
    cross = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
    dot = (ax * bx + ay * by) + mz * mz
    return np.arctan2(cross, dot) * RAD2DEG


def final(rows, coef, K, huber_mm=None):
    """The final pass at the solution -> dict: the 8 report numbers, inliers, used, max_shift."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    w = rows[:, 9]
    present = w > 0.0
    with np.errstate(all='ignore'):
        phi = phi_of(rows[:, 0], rows[:, 1])
        p = shift(phi, coef, K)
        xm, ym, tmx, tmy, e0, e1, e2 = (rows[:, i] for i in range(2, 9))
        ex, ey = tmx - xm, tmy - ym
        rx, ry = p[0] - ex, p[1] - ey
        r2 = rx * rx + ry * ry
        r = np.sqrt(r2)
        qx, qy = 0.0 - ex, 0.0 - ey                                       # the same at C = 0
        q2 = qx * qx + qy * qy
        q = np.sqrt(q2)
        _, _, inl = _huber(w, r2, r, huber_mm)
        mz = -e2
        deg = _angle((xm + p[0]) - e0, (ym + p[1]) - e1, tmx - e0, tmy - e1, mz)
        deg_raw = _angle((xm + 0.0) - e0, (ym + 0.0) - e1, tmx - e0, tmy - e1, mz)
        sh = np.sqrt(p[0] * p[0] + p[1] * p[1])
        contrib = np.stack([w * r2, w * r, inl, np.ones_like(w), w * deg, w * q2, w * q, w * deg_raw], axis=1)
    contrib[~present] = 0.0
    S = ordered_sums(contrib)
    mx = lambda a: float(np.max(np.where(a[present] > 0.0, a[present], 0.0))) if present.any() else 0.0      # a NaN never wins
    n = S[3]
    with np.errstate(all='ignore'):
        return {'rms_mm': float(np.sqrt(S[0] / n)), 'mean_mm': float(S[1] / n), 'max_mm': mx(r), 'mean_deg': float(S[4] / n),
                'rms_mm_raw': float(np.sqrt(S[5] / n)), 'mean_mm_raw': float(S[6] / n), 'max_mm_raw': mx(q), 'mean_deg_raw': float(S[7] / n),
                'inliers': int(S[2]), 'used': int(n), 'max_shift': mx(sh)}


def _result(kind, coef=None, ok=False, used=0, inliers=0, solves=0, report=None):
    out = {'coef': np.zeros((2, 6)) if coef is None or not ok else coef, 'kind': kind, 'ok': bool(ok), 'used': int(used),
           'inliers': int(inliers) if ok else 0, 'solves': int(solves) if ok else 0}
    for k in REPORT:
        out[k] = float(report[k]) if ok else 0.0
    return out


def fit(rows, kind, huber_mm=None, min_samples=None, max_shift_mm=100.0):
    """The header's schedule over rows [n, 12]: from C = 0, pass and solve; with huber_mm repeat until no coefficient moves by more
    than 1e-6 mm (at most 64 solves); the final pass; the refusals.  kind: 1 offset, 2 affine, 3 quadratic (or the name).  Where
    ok is False everything but `used` is 0."""
    kind = KINDS.get(kind, kind)
    K = terms_of(kind)
    assert K > 0
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    coef = np.zeros((2, 6))
    P = passes(rows, coef, K, huber_mm)
    used = int(P['n'])
    if used < max(1 if min_samples is None else int(min_samples), K) or not np.isfinite(P['cost']):
        return _result(kind, used=used)
    ok, coef = cholesky_solve(P['G'], P['bx'], P['by'], K)
    if not ok:
        return _result(kind, used=used)
    solves = 1
    if huber_mm is not None:
        while True:
            P = passes(rows, coef, K, huber_mm)
            ok, new = cholesky_solve(P['G'], P['bx'], P['by'], K)
            if not ok:
                return _result(kind, used=used)
            solves += 1
            with np.errstate(all='ignore'):
                step = 0.0
                for d in np.abs(new - coef).reshape(-1):
                    step = d if d > step else step
                converged = bool(np.isfinite(new).all()) and step <= STEP_TOL_MM
            coef = new
            if converged:
                break
            if solves == MAX_SOLVES:
                return _result(kind, used=used)
    F = final(rows, coef, K, huber_mm)
    if F['max_shift'] > float(max_shift_mm):
        return _result(kind, used=used)
    return _result(kind, coef, True, used, F['inliers'], solves, F)


def evaluate(rows, coef, kind):
    """Mode 1: the report of the stored map (coef [2, 6], kind 0 .. 3) over the rows; nothing is solved, no loss.  ok iff a row is
    present.  A map of kind 0 reports the raw numbers in both sets."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    K = terms_of(int(kind))
    coef = np.asarray(coef, dtype=np.float64).reshape(2, 6) if K else np.zeros((2, 6))
    F = final(rows, coef, K)
    return _result(int(kind), coef.copy(), F['used'] >= 1, F['used'], F['used'], 0, F)


def apply(px, ppm, coef, kind, screen_size):
    """px float32 [N, 2], ppm float32 [N, 2], one stream's coef [2, 6] and kind -> the corrected float32 [N, 2]; kind 0: the input."""
    px = np.asarray(px, dtype=np.float32).reshape(-1, 2)
    K = terms_of(int(kind))
    if K == 0:
        return px.copy()
    x, s = px.astype(np.float64), np.asarray(ppm).astype(np.float64).reshape(-1, 2)
    coef = np.asarray(coef, dtype=np.float64).reshape(2, 6)
    size = (float(screen_size[0]), float(screen_size[1]))
    with np.errstate(all='ignore'):
        u = (x[:, 0] + x[:, 0]) / size[0] - 1.0
        v = (x[:, 1] + x[:, 1]) / size[1] - 1.0
        p = shift(phi_of(u, v), coef, K)
        out = np.empty_like(x)
        for a in range(2):
            moved = x[:, a] + p[a] * s[:, a]
            out[:, a] = np.where(moved < 0.0, 0.0, np.where(moved > size[a], size[a], moved))
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- scenes
SCREEN = (1920, 1080)
PPM = (3.4, 3.5)
# a known map: about +-12 mm per term over the screen (u, v in -1 .. 1)
COEF_STAR = np.array([[9.0, -12.0, 7.0, 11.0, -8.0, 6.0], [-10.0, 8.0, 12.0, -7.0, 9.0, -11.0]])
NINE = [(u, v) for v in (-1.0, 0.0, 1.0) for u in (-1.0, 0.0, 1.0)]


def coef_star(model):
    c = np.zeros((2, 6))
    K = terms_of(KINDS[model])
    c[:, :K] = COEF_STAR[:, :K]
    return c


def map_error_mm(coef, kind, star, star_kind):
    """The longest difference of two maps' corrections over the nine points u, v in {-1, 0, 1}, millimetres."""
    u, v = np.array([p[0] for p in NINE]), np.array([p[1] for p in NINE])
    a, b = shift(phi_of(u, v), coef, terms_of(kind)), shift(phi_of(u, v), star, terms_of(star_kind))
    return float(np.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2).max())


def make_scene(seed, dots=(3, 3), per_dot=1, noise_mm=0.0, outliers=0, model='affine', outlier_mm=(80.0, 200.0), coef=None):
    """dots[0] x dots[1] targets between 10 % and 90 % of the screen, per_dot frames each; the raw points are the targets pushed
    through the inverse of the known map (coef, default coef_star(model)), + Gaussian noise of noise_mm per axis, the first
    `outliers` frames (after a shuffle) moved by outlier_mm[0] .. outlier_mm[1] in a random direction; pixels rounded to float32.
    -> dict(pog, origin, inv_cam, ppm, target, screen_size, coef, kind): float32 inputs of reduce()."""
    rng = np.random.RandomState(seed)
    kind = KINDS[model]
    K = terms_of(kind)
    star = coef_star(model) if coef is None else np.asarray(coef, dtype=np.float64)
    W, H = SCREEN
    span = lambda n, size: np.array([0.5 * size]) if n == 1 else np.linspace(0.1 * size, 0.9 * size, n)
    tx, ty = np.meshgrid(span(dots[0], W), span(dots[1], H))
    target = np.repeat(np.stack([tx.reshape(-1), ty.reshape(-1)], axis=1), per_dot, axis=0).astype(np.float32)
    n = target.shape[0]
    s = np.tile(np.asarray(PPM, dtype=np.float32), (n, 1))
    t64, s64 = target.astype(np.float64), s.astype(np.float64)
    x = t64.copy()
    for _ in range(60):                                                   # x + s(x) ppm = t by fixed-point iteration (a contraction)
        p = shift(phi_of((x[:, 0] + x[:, 0]) / W - 1.0, (x[:, 1] + x[:, 1]) / H - 1.0), star, K)
        x = t64 - np.stack(p, axis=1) * s64
    if noise_mm:
        x = x + rng.normal(0.0, noise_mm, x.shape) * s64
    if outliers:
        idx = rng.permutation(n)[:outliers]
        ang, dist = rng.uniform(0, 2 * np.pi, outliers), rng.uniform(outlier_mm[0], outlier_mm[1], outliers)
        x[idx] += np.stack([dist * np.cos(ang), dist * np.sin(ang)], axis=1) * s64[idx]
    origin = np.stack([rng.uniform(-80, 80, n), rng.uniform(-60, 60, n), rng.uniform(450, 750, n)], axis=1).astype(np.float32)
    inv_cam = np.zeros((n, 4, 4), dtype=np.float32)
    inv_cam[:, :3, :3] = _rot(rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.0).astype(np.float32)
    inv_cam[:, :3, 3] = np.array([260.0, 10.0, 0.0], dtype=np.float32)
    inv_cam[:, 3, 3] = 1.0
    return {'pog': x.astype(np.float32), 'origin': origin, 'inv_cam': inv_cam, 'ppm': s, 'target': target, 'screen_size': SCREEN,
            'coef': star, 'kind': kind}


def scene_rows(scene):
    rows, usable = reduce(scene['pog'], scene['origin'], scene['inv_cam'], scene['ppm'], scene['target'], scene['screen_size'])
    assert usable.all()
    return rows
