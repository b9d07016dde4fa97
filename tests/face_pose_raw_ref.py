"""The contract of eve_face_pose_solve_ex and eve_undistort_points (include/eve_hip.h) in numpy float64, the cases their tests
share, and stand-ins of HipKernels.face_pose_solve_ex / undistort_points for the torch-CPU FakeKernels.  The plain solve, its
cases and its helpers are tests/face_pose_ref.py's, by import; the forward lens model is tests/eye_warp_lens_ref.py's.

Two additions to the plain solve, both optional.  Every operation is rounded on its own in float64, in the association written
here, and every sum over the landmarks runs in landmark order from 0.0: only + - * / and sqrt occur.

POINT UNDISTORTION.  A lens row (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) (float32, widened) and a raw pixel (u, v):
    xd = (u - cx) / fx            yd = (v - cy) / fy
A row whose eight coefficients are all +-0 gives x = xd, y = yd, no iteration.  Otherwise Newton's method on distort(x, y) =
(xd, yd) from (x, y) = (xd, yd); one step is
    xx = x*x   yy = y*y   xy = x*y   r2 = xx + yy
    N  = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0            D  = ((k6*r2 + k5)*r2 + k4)*r2 + 1.0
    rad = N / D                   a = xy + xy
    gx = (x*rad + p1*a) + p2*(r2 + (xx + xx))       gy = (y*rad + p1*(r2 + (yy + yy))) + p2*a         (eye_warp_lens_ref's distort)
    N' = ((3.0*k3)*r2 + 2.0*k2)*r2 + k1             D' = ((3.0*k6)*r2 + 2.0*k5)*r2 + k4
    rp = (N' - rad*D') / D        tw = rp + rp
    j00 = ((rad + xx*tw) + 2.0*(p1*y)) + 6.0*(p2*x)
    j01 = (xy*tw + 2.0*(p1*x)) + 2.0*(p2*y)                                                           (= j10)
    j11 = ((rad + yy*tw) + 6.0*(p1*y)) + 2.0*(p2*x)
    ex = gx - xd   ey = gy - yd   det = j00*j11 - j01*j01
    dx = (j11*ex - j01*ey) / det  dy = (j00*ey - j01*ex) / det
    dx or dy not finite: the point is unusable.  x = x - dx, y = y - dy;
    max(|dx|, |dy|) <= 4e-15 * max(1.0, |x|, |y|) (the new x, y): done.
Twelve steps without that: unusable.  At the result D is evaluated once more (xx, yy, r2, D as above): not D > 0: unusable.
Uniqueness is not promised beyond the fold-back radius of a barrel polynomial -- the pixel warp's unguarded case.

In the solve a frame's lens row undistorts its landmarks and the solve continues from (x, y) directly; the rig's fx .. cy keep
their roles (the pix column, the normalisation that follows).  An unusable point is dropped: w = 0, x = y = 0.0, not used.  A
lens row with a non-finite entry or fx <= 0 or fy <= 0 makes the frame invalid, like a non-finite landmark.

HUBER LOSS, huber_px = k > 0 (pixels).  Per used point, from the plain contract's ex, ey, Jx, Jy:
    p2 = (fx*ex)*(fx*ex) + (fy*ey)*(fy*ey)          r = sqrt(p2)          inlier iff not r > k
    s = 1.0 for an inlier, else k / r               ws = w * s
    A_ij = ws * (Jx_i*Jx_j + Jy_i*Jy_j)             g_i = ws * (Jx_i*ex + Jy_i*ey)
    cost = w * (p2 if inlier else k*((r + r) - k))  pix = w * p2          a 30th column: 1.0 for an inlier
The iteration, the damping, the accept test (on the cost column), small, the cap and the observability Cholesky are the plain
contract's.  A frame that converges with fewer than 4 inliers is invalid.  Without the loss the 29 plain columns stand.

OUTPUTS as the plain solve's, plus inliers uint8: the 30th column's sum with the loss, the number of used points without, 0 on
an invalid frame.  reproj_rms = sqrt(pix / sw) over all used points, weighted by w.  No lens and no loss: face_pose_ref.solve's
bits.  Not promised: L = 6 with an outlier (a Huber loss cannot tell which of six points is wrong)."""
import numpy as np
import torch

import eye_pose_ref as pref
import eye_warp_lens_ref as lref
import face_pose_ref as fr

NC = 30
MAX_NEWTON = 12
# the issue's four lenses: coefficient tuples in OpenCV's order (k1, k2, p1, p2, k3[, k4, k5, k6])
LENS_COEFFS = {
    'barrel5': (-0.35, 0.15, 1e-3, -5e-4, -0.03),
    'pincushion4': (0.08, -0.02, 5e-4, 3e-4),
    'rational8': (2.5, 1.2, 1e-3, -5e-4, 0.1, 2.8, 1.6, 0.3),
    'barrel3': (-0.28, 0.07, 0.0, 0.0, -0.006),
}


def lens_row(coeffs, K=fr.CAMERA):
    c = list(coeffs) + [0.0] * (8 - len(coeffs))
    return np.array(list(K) + c, dtype=np.float32)


LENSES = {name: lens_row(c) for name, c in LENS_COEFFS.items()}


def lens_usable(row):
    r = np.asarray(row, dtype=np.float64)
    return bool(np.isfinite(r).all() and r[0] > 0 and r[1] > 0)


def distort_normalized(x, y, row):
    """The forward model on normalised coordinates in the contract's association -> (gx, gy)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(t) for t in np.asarray(row)[4:])
    with np.errstate(all='ignore'):
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        rad = (((k3 * r2 + k2) * r2 + k1) * r2 + 1.0) / (((k6 * r2 + k5) * r2 + k4) * r2 + 1.0)
        a = xy + xy
        return (x * rad + p1 * a) + p2 * (r2 + (xx + xx)), (y * rad + p1 * (r2 + (yy + yy))) + p2 * a


def undistort(u, v, row):
    """u, v float64 [n] raw pixels, row 12 values (a usable lens row) -> (x, y float64 [n] normalised, zero where not ok; ok bool
    [n]; steps int [n])."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(t) for t in row)
    u, v = np.atleast_1d(np.asarray(u, dtype=np.float64)), np.atleast_1d(np.asarray(v, dtype=np.float64))
    n = u.shape[0]
    with np.errstate(all='ignore'):
        xd, yd = (u - cx) / fx, (v - cy) / fy
        if lref.takes_the_plain_path(row):
            return xd, yd, np.ones(n, dtype=bool), np.zeros(n, dtype=np.int64)
        x, y = xd.copy(), yd.copy()
        active, ok, steps = np.ones(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
        for _ in range(MAX_NEWTON):
            xx, yy, xy = x * x, y * y, x * y
            r2 = xx + yy
            N = ((k3 * r2 + k2) * r2 + k1) * r2 + 1.0
            D = ((k6 * r2 + k5) * r2 + k4) * r2 + 1.0
            rad, a = N / D, xy + xy
            gx = (x * rad + p1 * a) + p2 * (r2 + (xx + xx))
            gy = (y * rad + p1 * (r2 + (yy + yy))) + p2 * a
            Np = ((3.0 * k3) * r2 + 2.0 * k2) * r2 + k1
            Dp = ((3.0 * k6) * r2 + 2.0 * k5) * r2 + k4
            rp = (Np - rad * Dp) / D
            tw = rp + rp
            j00 = ((rad + xx * tw) + 2.0 * (p1 * y)) + 6.0 * (p2 * x)
            j01 = (xy * tw + 2.0 * (p1 * x)) + 2.0 * (p2 * y)
            j11 = ((rad + yy * tw) + 6.0 * (p1 * y)) + 2.0 * (p2 * x)
            ex, ey = gx - xd, gy - yd
            det = j00 * j11 - j01 * j01
            dx, dy = (j11 * ex - j01 * ey) / det, (j00 * ey - j01 * ex) / det
            upd = active & np.isfinite(dx) & np.isfinite(dy)
            x, y = np.where(upd, x - dx, x), np.where(upd, y - dy, y)
            steps = steps + upd
            done = upd & (np.maximum(np.abs(dx), np.abs(dy)) <= 4e-15 * np.maximum(1.0, np.maximum(np.abs(x), np.abs(y))))
            ok = ok | done
            active = upd & ~done
            if not active.any():
                break
        xx, yy = x * x, y * y
        r2 = xx + yy
        ok = ok & (((k6 * r2 + k5) * r2 + k4) * r2 + 1.0 > 0)
        return np.where(ok, x, 0.0), np.where(ok, y, 0.0), ok, steps


def undistort_points(points, lens):
    """The contract of eve_undistort_points: points float32 [N, 2], lens float32 [N, 12] or [1, 12] -> (xy float64 [N, 2]
    normalised, ok uint8 [N]).  ok = 0 and xy = 0 for a non-finite point, a lens row that is not usable, an unusable point."""
    points, lens = np.asarray(points), np.asarray(lens)
    assert points.dtype == np.float32 and points.ndim == 2 and points.shape[1] == 2, (points.dtype, points.shape)
    N = points.shape[0]
    assert lens.dtype == np.float32 and lens.shape in ((N, 12), (1, 12)), (lens.dtype, lens.shape)
    xy, ok = np.zeros((N, 2)), np.zeros(N, dtype=np.uint8)
    p = points.astype(np.float64)
    rows = np.broadcast_to(lens, (N, 12))
    # points that share a row are done together (elementwise: the same bits as one by one)
    _, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    for g, i in enumerate(first):
        idx = np.nonzero(inverse == g)[0]
        if not lens_usable(rows[i]):
            continue
        fin = np.isfinite(p[idx]).all(axis=1)
        idx = idx[fin]
        if idx.size == 0:
            continue
        x, y, good, _ = undistort(p[idx, 0], p[idx, 1], rows[i])
        xy[idx, 0], xy[idx, 1], ok[idx] = x, y, good
    return xy, ok


# ------------------------------------------------------------------------------------------------ the solve
def evaluate_huber(R, t, X, x, y, w, used, fx, fy, k):
    """-> (the 30 sums, behind)"""
    with np.errstate(all='ignore'):
        q = [(R[i][0] * X[:, 0] + R[i][1] * X[:, 1]) + R[i][2] * X[:, 2] for i in range(3)]
        P = [q[i] + t[i] for i in range(3)]
        iz = 1.0 / P[2]
        px, py = P[0] / P[2], P[1] / P[2]
        ex, ey = px - x, py - y
        a, b = px * iz, py * iz
        zero = np.zeros_like(iz)
        Jx = [-(a * q[1]), iz * q[2] + a * q[0], -(iz * q[1]), iz, zero, -a]
        Jy = [-(iz * q[2] + b * q[1]), b * q[0], iz * q[0], zero, iz, -b]
        p2 = (fx * ex) * (fx * ex) + (fy * ey) * (fy * ey)
        r = np.sqrt(p2)
        inlier = ~(r > k)
        ws = w * np.where(inlier, 1.0, k / r)
        cols = [ws * (Jx[i] * Jx[j] + Jy[i] * Jy[j]) for i in range(6) for j in range(i, 6)]
        cols += [ws * (Jx[i] * ex + Jy[i] * ey) for i in range(6)]
        cols.append(w * np.where(inlier, p2, k * ((r + r) - k)))
        cols.append(w * p2)
        cols.append(np.where(inlier, 1.0, 0.0))
        c = np.where(used[:, None], np.stack(cols, axis=-1), 0.0)
        behind = bool((used & ~(P[2] > 0)).any())
    return fr.ordered_sum(c), behind


def solve_frame(lm, rig, lens=None, huber_px=None, init=None):
    """One frame: lm float32 [L, 2 | 3], rig float32 [12 + 3L], lens None or float32 [12], huber_px None or k > 0, init None (cold)
    or (R, t) float64 -> dict(valid, R, t float64, rms float64, inliers, accepted, evals, newton (most steps of a point))."""
    L = lm.shape[0]
    bad = dict(valid=False, R=fr.I3.copy(), t=np.zeros(3), rms=0.0, inliers=0, accepted=0, evals=0, newton=0)
    r = rig.astype(np.float64)
    fx, fy, cx, cy = r[0], r[1], r[2], r[3]
    X = r[12:].reshape(L, 3)
    p = lm.astype(np.float64)
    if not (np.isfinite(r).all() and np.isfinite(p).all() and fx > 0 and fy > 0):
        return bad
    if lens is not None and not lens_usable(lens):
        return bad
    w = p[:, 2] if p.shape[1] == 3 else np.ones(L)
    used = w > 0
    newton = 0
    if lens is None:
        x, y = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    else:
        x, y, ok, steps = undistort(p[:, 0], p[:, 1], lens)
        used, newton = used & ok, int(steps.max())
    w = np.where(used, w, 0.0)
    if used.sum() < 4:
        return bad
    sw = fr.ordered_sum(w[:, None])[0]
    if init is None:
        init = fr.cold_start(X, x, y, w)
        if init is None:
            return bad
    if huber_px is None:
        ev = lambda R_, t_: fr.evaluate(R_, t_, X, x, y, w, used, fx, fy)
    else:
        ev = lambda R_, t_: evaluate_huber(R_, t_, X, x, y, w, used, fx, fy, np.float64(huber_px))
    R, t = np.array(init[0], dtype=np.float64), np.array(init[1], dtype=np.float64)
    S, behind = ev(R, t)
    evals = 1
    if behind or not np.isfinite(S[27]):
        return bad
    lam, accepted, converged = 1e-3, 0, False
    while not converged:
        A, g, cost, _ = fr.unpack(S)
        M = A.copy()
        for i in range(6):
            M[i][i] = A[i][i] + lam * A[i][i]
        Lo = fr.cholesky(M, 0.0)
        if Lo is None:
            return bad
        d = fr.chol_solve(Lo, -g)
        finite = bool(np.isfinite(d).all())
        Rc, tc = fr.cayley_update(R, d), t + d[3:6]
        Sc, behind = ev(Rc, tc)
        evals += 1
        small = finite and np.abs(d).max() < 1e-10 * max(1.0, np.abs(t).max())
        if finite and not behind and Sc[27] <= cost:
            R, t, S = Rc, tc, Sc
            lam = lam / 10.0
            accepted += 1
            if small:
                converged = True
            elif accepted == 32:
                return bad
        elif small:
            converged = True
        else:
            lam = lam * 10.0
            if lam > 1e12:
                return bad
    A, _, _, pix = fr.unpack(S)
    if fr.cholesky(A, 1e-10) is None:
        return bad
    inliers = int(used.sum()) if huber_px is None else int(S[29])
    if inliers < 4:
        return bad
    with np.errstate(all='ignore'):
        rms = np.sqrt(pix / sw)
    return dict(valid=True, R=R, t=t, rms=rms, inliers=inliers, accepted=accepted, evals=evals, newton=newton)


def solve(landmarks, rig, lens=None, huber_px=None, lengths=None, state=None, reset=None):
    """face_pose_ref.solve with lens None or float32 [S, T, 12] and huber_px None or k > 0; the dict gains inliers uint8 [S, T]."""
    landmarks, rig = np.asarray(landmarks), np.asarray(rig)
    assert landmarks.dtype == np.float32 and landmarks.ndim == 4 and landmarks.shape[3] in (2, 3), (landmarks.dtype, landmarks.shape)
    S, T, L = landmarks.shape[:3]
    assert rig.dtype == np.float32 and rig.shape == (S, 12 + 3 * L), (rig.dtype, rig.shape)
    if lens is not None:
        lens = np.asarray(lens)
        assert lens.dtype == np.float32 and lens.shape == (S, T, 12), (lens.dtype, lens.shape)
    out = dict(head_R=np.zeros((S, T, 3, 3), np.float32), head_t=np.zeros((S, T, 3), np.float32), reproj_rms=np.zeros((S, T), np.float32),
               valid=np.zeros((S, T), np.uint8), inliers=np.zeros((S, T), np.uint8), accepted=np.zeros((S, T), np.int64))
    out['head_R'][:] = np.eye(3, dtype=np.float32)
    for s in range(S):
        n = T if lengths is None else min(max(int(lengths[s]), 0), T)
        pose, dirty = None, False
        if state is not None and state[s, 12] != 0:
            pose = (state[s, :9].reshape(3, 3).copy(), state[s, 9:12].copy())
        if reset is not None and reset[s] != 0:
            pose, dirty = None, True
        for t in range(n):
            res = solve_frame(landmarks[s, t], rig[s], None if lens is None else lens[s, t], huber_px, pose)
            dirty = True
            pose = (res['R'], res['t']) if res['valid'] else None
            out['valid'][s, t], out['accepted'][s, t], out['inliers'][s, t] = res['valid'], res['accepted'], res['inliers']
            if res['valid']:
                out['head_R'][s, t], out['head_t'][s, t], out['reproj_rms'][s, t] = pref.f32(res['R']), pref.f32(res['t']), pref.f32(res['rms'])
        if state is not None and dirty:
            state[s] = np.concatenate([fr.I3.reshape(-1), np.zeros(4)]) if pose is None else np.concatenate([pose[0].reshape(-1), pose[1], [1.0]])
    return out


# ------------------------------------------------------------------------------------------------ the shared cases
def angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, dtype=np.float64) @ np.asarray(Rb, dtype=np.float64).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def contaminated_case(L, nout, seed):
    """The issue's robustness recipe: face_pose_ref's cold case at 1 px noise, then nout landmarks moved 30..80 px in a uniform
    random direction -> (model, clean float32 [L, 2], contaminated float32 [L, 2], R, t, the moved indices)."""
    g = np.random.default_rng(seed)
    model = fr.head_model(L, seed)
    R, t = fr.random_pose(g)
    clean = fr.project(model, R, t, g=g)
    lm = clean.astype(np.float64)
    idx = g.choice(L, nout, replace=False)
    ang, mag = g.uniform(0, 2 * np.pi, nout), g.uniform(30, 80, nout)
    lm[idx, 0] += mag * np.cos(ang)
    lm[idx, 1] += mag * np.sin(ang)
    return model, clean, lm.astype(np.float32), R, t, idx


def distort_landmarks(lm, row):
    """float32 landmarks [..., L, 2 | 3] of the undistorted image -> the raw frame's, float32 (the weight column kept)."""
    lm = np.asarray(lm)
    ud, vd, _ = lref.distort(lm[..., 0].astype(np.float64), lm[..., 1].astype(np.float64), row)
    out = lm.copy()
    out[..., 0], out[..., 1] = ud, vd
    return out


def raw_sequences(S, T, L, seed, weights=False, lens_names=('barrel5', 'rational8', 'pincushion4'), **kw):
    """face_pose_ref.sequences distorted: sequence s through lens lens_names[s % ...] -> (raw landmarks float32 [S, T, L, 2 | 3],
    rig float32 [S, 12 + 3L], lens float32 [S, T, 12], the undistorted landmarks)."""
    lm, rig = fr.sequences(S, T, L, seed, weights=weights, **kw)
    lens = np.stack([np.stack([LENSES[lens_names[s % len(lens_names)]]] * T) for s in range(S)])
    raw = np.stack([distort_landmarks(lm[s], lens[s, 0]) for s in range(S)])
    return raw, rig, lens, lm


# ------------------------------------------------------------------------------------------------ stand-ins for FakeKernels
def face_pose_solve_ex(self, landmarks, rig, lens=None, huber_px=None, lengths=None, state=None, reset=None):
    """Stand-in of HipKernels.face_pose_solve_ex."""
    if not torch.is_tensor(landmarks) or landmarks.dtype != torch.float32 or landmarks.dim() != 4 or landmarks.shape[3] not in (2, 3):
        raise TypeError('face_pose_solve_ex: landmarks must be float32 [S, T, L, 2 | 3]')
    S, T, L = landmarks.shape[:3]
    if not torch.is_tensor(rig) or rig.dtype != torch.float32 or tuple(rig.shape) != (S, 12 + 3 * L):
        raise TypeError('face_pose_solve_ex: rig must be float32 [S, 12 + 3 L]')
    if lens is not None and (not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) != (S, T, 12)):
        raise TypeError('face_pose_solve_ex: lens must be float32 [S, T, 12]')
    if huber_px is not None and not float(huber_px) > 0:
        raise ValueError('face_pose_solve_ex: huber_px must be None or > 0')
    opt = lambda t: None if t is None else t.numpy()
    res = solve(landmarks.numpy(), rig.numpy(), opt(lens), None if huber_px is None else float(huber_px), opt(lengths), opt(state), opt(reset))
    return tuple(torch.from_numpy(res[k_]) for k_ in ('head_R', 'head_t', 'reproj_rms', 'valid', 'inliers'))


def undistort_points_fake(self, points, lens):
    """Stand-in of HipKernels.undistort_points."""
    if not torch.is_tensor(points) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 2:
        raise TypeError('undistort_points: points must be float32 [N, 2]')
    if not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) not in ((points.shape[0], 12), (1, 12)):
        raise TypeError('undistort_points: lens must be float32 [N, 12] or [1, 12]')
    xy, ok = undistort_points(points.numpy(), lens.numpy())
    return torch.from_numpy(xy), torch.from_numpy(ok)
