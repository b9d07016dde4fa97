"""The contract of eve_face_pose_solve (include/eve_hip.h) in numpy float64, the cases the tests share, the continuation of
tests/eye_pose_ref.py from a solved (head_R, head_t) -- the contract of eve_eye_pose_normalize_rt -- and stand-ins of
HipKernels.face_pose_solve / eye_pose_normalize_rt for the torch-CPU FakeKernels.

A weighted perspective-n-point solve by Levenberg-Marquardt on the reprojection error in normalised image coordinates, one frame
after the other, warm-started from the previous frame.  Every operation is rounded on its own (numpy evaluates every ufunc on
its own), in the association written below, and every sum over the landmarks is taken in landmark order 0 .. L-1 from 0.0 by a
plain loop: only + - * / and sqrt occur, each correctly rounded, so the device's float64 results are these bits.

  rig row (float32, widened)  (fx, fy, cx, cy, left eye centre, right eye centre, focal_norm, distance_norm, X_0 .. X_{L-1})
  landmark l of a frame       (u, v[, w]);  x = (u - cx) / fx,  y = (v - cy) / fy,  w = 1.0 without the column; used iff w > 0
  eval(R, t), per used point  q_i = (R[i][0]*X0 + R[i][1]*X1) + R[i][2]*X2,  P = q + t,  iz = 1.0 / P2,  px = P0 / P2,  py = P1 / P2,
                              ex = px - x, ey = py - y, a = px * iz, b = py * iz,
                              Jx = (-(a*q1), iz*q2 + a*q0, -(iz*q1), iz, 0.0, -a)
                              Jy = (-(iz*q2 + b*q1), b*q0, iz*q0, 0.0, iz, -b)
                              29 columns: A_ij = w * (Jx_i*Jx_j + Jy_i*Jy_j) for i <= j, row-major (21); g_i = w * (Jx_i*ex + Jy_i*ey)
                              (6); cost = w * (ex*ex + ey*ey); pix = w * ((fx*ex)*(fx*ex) + (fy*ey)*(fy*ey)).  An unused point
                              contributes 0.0 to every column.  behind = a used point with not P2 > 0.
  cold start                  sw = sum w, (mx, my, MX, MY, MZ) = sum(w * (x, y, X0, X1, X2)) / sw,
                              sl = sum w * ((x-mx)*(x-mx) + (y-my)*(y-my)),  sm = sum w * ((X0-MX)*(X0-MX) + (X1-MY)*(X1-MY)),
                              not (sl > 0 and sm > 0): invalid; Z = sqrt(sm / sl), R = I, t = (mx*Z - MX, my*Z - MY, Z - MZ)
  iteration                   lam = 1e-3, accepted = 0, S = eval(R, t); behind, or a cost that is not finite: invalid.  Then
                              M = A, M_ii = A_ii + lam * A_ii; Cholesky (below, thr = 0) of M, d = solve(M, -g); a failed pivot:
                              invalid.  a = 0.5 * d[0:3], s = (a0*a0 + a1*a1) + a2*a2, den = 1.0 + s, e = 1.0 - s,
                              C = [[(e + 2.0*(a0*a0))/den, (2.0*(a0*a1 - a2))/den, (2.0*(a0*a2 + a1))/den],
                                   [(2.0*(a0*a1 + a2))/den, (e + 2.0*(a1*a1))/den, (2.0*(a1*a2 - a0))/den],
                                   [(2.0*(a0*a2 - a1))/den, (2.0*(a1*a2 + a0))/den, (e + 2.0*(a2*a2))/den]]      (the Cayley map)
                              Rc[i][j] = (C[i][0]*R[0][j] + C[i][1]*R[1][j]) + C[i][2]*R[2][j], tc = t + d[3:6], Sc = eval(Rc, tc)
                              small = every d_i finite and max|d_i| < 1e-10 * max(1.0, max|t_i|)         (t before the update)
                              accept iff every d_i finite, not behind and cost_c <= cost: (R, t, S) = (Rc, tc, Sc), lam = lam / 10.0,
                              accepted += 1; small: converged; else accepted == 32: invalid.  Rejected: small: converged (the
                              pose as it was); else lam = lam * 10.0, lam > 1e12: invalid.
  observability               converged: one more Cholesky of the undamped A with thr = 1e-10; a failed pivot: invalid (the
                              landmarks do not determine the pose: collinear model points, say).
  Cholesky(M, thr)            for j: s = M_jj; for k < j: s = s - L_jk*L_jk; not s > thr * M_jj: failed; L_jj = sqrt(s);
                              for i > j: s = M_ij; for k < j: s = s - L_ik*L_jk; L_ij = s / L_jj
                              y_i = (b_i - sum_{k<i} L_ik*y_k) / L_ii (subtracted one by one, k rising), x_i = (y_i - sum_{k>i}
                              L_ki*x_k) / L_ii (i falling, k rising)
  outputs                     head_R = float32(R), head_t = float32(t), reproj_rms = float32(sqrt(pix / sw)); an invalid frame:
                              R = I, t = 0, rms = 0, valid = 0.
  invalid before any of it    a non-finite rig entry or landmark (u, v or w, of a used point or not), fx <= 0 or fy <= 0, fewer
                              than 4 used points.
  sequence                    frame 0 starts from the carried state (R, t, has_pose) if has_pose != 0 and no reset is flagged,
                              every later frame from the previous frame's float64 solution if that frame was valid, else cold.
                              Frames at t >= lengths[s] are not solved, are reported invalid and leave the carried pose alone; a
                              solved invalid frame (and a reset) clears it to (I, 0, 0); a valid one sets (R, t, 1)."""
import numpy as np
import torch

import eye_pose_ref as pref

NC = 29
MODEL_SIZES = (6, 7, 64, 65, 68)
FOCAL = 1000.0
CAMERA = (FOCAL, FOCAL, 640.0, 360.0)
EYES = ((-32.0, -35.0, 25.0), (32.0, -35.0, 25.0))
FOCAL_NORM, DISTANCE_NORM = 220.0, 600.0
I3 = np.eye(3)


# ------------------------------------------------------------------------------------------------ the shared cases
def head_model(L, seed):
    """A non-planar head model: x, y within +-70, z within +-30 -> float32 [L, 3]."""
    g = np.random.default_rng(1000 + seed)
    return np.stack([g.uniform(-70, 70, L), g.uniform(-70, 70, L), g.uniform(-30, 30, L)], axis=-1).astype(np.float32)


def rot_xyz(pitch, yaw, roll):
    cx, sx, cy, sy, cz, sz = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def random_pose(g):
    """pitch, yaw within +-40 degrees, roll within +-20, t = (+-150, +-100, 350..900) -> (R [3, 3], t [3]) float64."""
    d = np.pi / 180.0
    R = rot_xyz(g.uniform(-40, 40) * d, g.uniform(-40, 40) * d, g.uniform(-20, 20) * d)
    return R, np.array([g.uniform(-150, 150), g.uniform(-100, 100), g.uniform(350, 900)])


def project(model, R, t, K=CAMERA, noise=1.0, g=None, weights=None):
    """float32 landmarks [L, 2 | 3] of the model under (R, t), with `noise` px of Gaussian noise."""
    P = model.astype(np.float64) @ R.T + t
    uv = np.stack([K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]], axis=-1)
    if noise:
        uv = uv + g.normal(0.0, noise, uv.shape)
    if weights is not None:
        uv = np.concatenate([uv, np.asarray(weights, dtype=np.float64)[:, None]], axis=-1)
    return uv.astype(np.float32)


def rig_row(model, K=CAMERA, eyes=EYES, focal_norm=FOCAL_NORM, distance_norm=DISTANCE_NORM):
    return np.array(list(K) + list(eyes[0]) + list(eyes[1]) + [focal_norm, distance_norm] + list(np.asarray(model).reshape(-1)),
                    dtype=np.float32)


def case(L, seed, weights=False):
    """One cold case of the issue: (model float32 [L, 3], landmarks float32 [L, 2 | 3], R, t)."""
    g = np.random.default_rng(seed)
    model = head_model(L, seed)
    R, t = random_pose(g)
    w = g.uniform(0.2, 1.0, L) if weights else None
    return model, project(model, R, t, g=g, weights=w), R, t


def sequences(S, T, L, seed, weights=False, step_deg=3.0, step_mm=8.0, K=CAMERA, frontal=False, focal_norm=FOCAL_NORM, noise=1.0):
    """S sequences of T frames: each starts at a random pose of the issue (a cold start at up to +-40 degrees) and then moves by
    up to step_deg degrees per axis and step_mm per frame -> (landmarks float32 [S, T, L, 2 | 3], rig float32 [S, 12 + 3L]).
    frontal: within +-15 degrees at (+-30, +-20, 500..700) instead, for the end-to-end cases whose patches should look into a
    small frame of camera K.  noise: in pixels -- 1 px at the issue's f = 1000; a shorter focal length wants it scaled down with
    it, because the solve's convergence is linear at a rate set by the noise relative to the face's size in the image, and the
    contract's cap of 32 accepted steps turns a frame with several per cent of noise into an invalid one."""
    g = np.random.default_rng(seed)
    lm, rig = [], []
    for s in range(S):
        model = head_model(L, seed * 31 + s)
        R, t = random_pose(g)
        if frontal:
            R = rot_xyz(*(g.uniform(-15, 15, 3) * np.pi / 180.0))
            t = np.array([g.uniform(-30, 30), g.uniform(-20, 20), g.uniform(500, 700)])
        frames = []
        for _ in range(T):
            frames.append(project(model, R, t, K=K, noise=noise, g=g, weights=g.uniform(0.2, 1.0, L) if weights else None))
            dr = g.uniform(-step_deg, step_deg, 3) * np.pi / 180.0
            R = rot_xyz(*dr) @ R
            t = t + g.uniform(-step_mm, step_mm, 3)
        lm.append(np.stack(frames))
        rig.append(rig_row(model, K=K, focal_norm=focal_norm))
    return np.stack(lm), np.stack(rig)


def planar_sequences(S, T, seed):
    """L = 4, a planar model (a bit-exactness case only: which of a planar model's two minima is found is not promised)."""
    g = np.random.default_rng(seed)
    model = np.array([[-60, -40, 0], [60, -40, 0], [60, 40, 0], [-60, 40, 0]], dtype=np.float32)
    lm = []
    for s in range(S):
        R, t = random_pose(g)
        lm.append(np.stack([project(model, R, t, g=g) for _ in range(T)]))
    return np.stack(lm), np.stack([rig_row(model)] * S)


# ------------------------------------------------------------------------------------------------ the contract
def ordered_sum(c):
    """c float64 [L, n] -> the n sums over the rows, taken in row order from 0.0."""
    s = np.zeros(c.shape[1])
    for l in range(c.shape[0]):
        s = s + c[l]
    return s


def evaluate(R, t, X, x, y, w, used, fx, fy):
    """-> (the 29 sums, behind)"""
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
        cols = [w * (Jx[i] * Jx[j] + Jy[i] * Jy[j]) for i in range(6) for j in range(i, 6)]
        cols += [w * (Jx[i] * ex + Jy[i] * ey) for i in range(6)]
        cols.append(w * (ex * ex + ey * ey))
        cols.append(w * ((fx * ex) * (fx * ex) + (fy * ey) * (fy * ey)))
        c = np.where(used[:, None], np.stack(cols, axis=-1), 0.0)
        behind = bool((used & ~(P[2] > 0)).any())
    return ordered_sum(c), behind


def unpack(S):
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = S[k]
            k += 1
    return A, S[21:27], S[27], S[28]


def cholesky(M, thr):
    """-> the lower factor, or None where a pivot fails."""
    Lo = np.zeros((6, 6))
    with np.errstate(all='ignore'):
        for j in range(6):
            s = M[j][j]
            for k in range(j):
                s = s - Lo[j][k] * Lo[j][k]
            if not s > thr * M[j][j]:
                return None
            Lo[j][j] = np.sqrt(s)
            for i in range(j + 1, 6):
                s = M[i][j]
                for k in range(j):
                    s = s - Lo[i][k] * Lo[j][k]
                Lo[i][j] = s / Lo[j][j]
    return Lo


def chol_solve(Lo, b):
    yv, xv = np.zeros(6), np.zeros(6)
    with np.errstate(all='ignore'):
        for i in range(6):
            s = b[i]
            for k in range(i):
                s = s - Lo[i][k] * yv[k]
            yv[i] = s / Lo[i][i]
        for i in range(5, -1, -1):
            s = yv[i]
            for k in range(i + 1, 6):
                s = s - Lo[k][i] * xv[k]
            xv[i] = s / Lo[i][i]
    return xv


def cayley_update(R, d):
    with np.errstate(all='ignore'):
        a0, a1, a2 = 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]
        s = (a0 * a0 + a1 * a1) + a2 * a2
        den, e = 1.0 + s, 1.0 - s
        C = [[(e + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1 - a2)) / den, (2.0 * (a0 * a2 + a1)) / den],
             [(2.0 * (a0 * a1 + a2)) / den, (e + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2 - a0)) / den],
             [(2.0 * (a0 * a2 - a1)) / den, (2.0 * (a1 * a2 + a0)) / den, (e + 2.0 * (a2 * a2)) / den]]
        return np.array([[(C[i][0] * R[0][j] + C[i][1] * R[1][j]) + C[i][2] * R[2][j] for j in range(3)] for i in range(3)])


def cold_start(X, x, y, w):
    """-> (R, t) or None"""
    with np.errstate(all='ignore'):
        s1 = ordered_sum(np.stack([w, w * x, w * y, w * X[:, 0], w * X[:, 1], w * X[:, 2]], axis=-1))
        sw = s1[0]
        mx, my, MX, MY, MZ = s1[1] / sw, s1[2] / sw, s1[3] / sw, s1[4] / sw, s1[5] / sw
        s2 = ordered_sum(np.stack([w * ((x - mx) * (x - mx) + (y - my) * (y - my)),
                                   w * ((X[:, 0] - MX) * (X[:, 0] - MX) + (X[:, 1] - MY) * (X[:, 1] - MY))], axis=-1))
        if not (s2[0] > 0 and s2[1] > 0):
            return None
        Z = np.sqrt(s2[1] / s2[0])
        return I3.copy(), np.array([mx * Z - MX, my * Z - MY, Z - MZ])


def solve_frame(lm, rig, init=None):
    """One frame: lm float32 [L, 2 | 3], rig float32 [12 + 3L], init None (cold) or (R, t) float64 -> dict(valid, R, t float64,
    rms float64, accepted, evals); R = I, t = 0, rms = 0 where invalid."""
    L = lm.shape[0]
    bad = dict(valid=False, R=I3.copy(), t=np.zeros(3), rms=0.0, accepted=0, evals=0)
    r = rig.astype(np.float64)
    fx, fy, cx, cy = r[0], r[1], r[2], r[3]
    X = r[12:].reshape(L, 3)
    p = lm.astype(np.float64)
    if not (np.isfinite(r).all() and np.isfinite(p).all() and fx > 0 and fy > 0):
        return bad
    w = p[:, 2] if p.shape[1] == 3 else np.ones(L)
    used = w > 0
    w = np.where(used, w, 0.0)
    if used.sum() < 4:
        return bad
    x, y = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    sw = ordered_sum(w[:, None])[0]
    if init is None:
        init = cold_start(X, x, y, w)
        if init is None:
            return bad
    R, t = np.array(init[0], dtype=np.float64), np.array(init[1], dtype=np.float64)
    S, behind = evaluate(R, t, X, x, y, w, used, fx, fy)
    evals = 1
    if behind or not np.isfinite(S[27]):
        return bad
    lam, accepted, converged = 1e-3, 0, False
    while not converged:
        A, g, cost, _ = unpack(S)
        M = A.copy()
        for i in range(6):
            M[i][i] = A[i][i] + lam * A[i][i]
        Lo = cholesky(M, 0.0)
        if Lo is None:
            return bad
        d = chol_solve(Lo, -g)
        finite = bool(np.isfinite(d).all())
        Rc, tc = cayley_update(R, d), t + d[3:6]
        Sc, behind = evaluate(Rc, tc, X, x, y, w, used, fx, fy)
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
    A, _, _, pix = unpack(S)
    if cholesky(A, 1e-10) is None:
        return bad
    with np.errstate(all='ignore'):
        rms = np.sqrt(pix / sw)
    return dict(valid=True, R=R, t=t, rms=rms, accepted=accepted, evals=evals)


def solve(landmarks, rig, lengths=None, state=None, reset=None):
    """landmarks float32 [S, T, L, 2 | 3], rig float32 [S, 12 + 3L], lengths None or int [S], state None or float64 [S, 13]
    (UPDATED IN PLACE), reset None or int [S] -> dict(head_R float32 [S, T, 3, 3], head_t float32 [S, T, 3], reproj_rms float32
    [S, T], valid uint8 [S, T], accepted int [S, T])."""
    landmarks, rig = np.asarray(landmarks), np.asarray(rig)
    assert landmarks.dtype == np.float32 and landmarks.ndim == 4 and landmarks.shape[3] in (2, 3), (landmarks.dtype, landmarks.shape)
    S, T, L = landmarks.shape[:3]
    assert rig.dtype == np.float32 and rig.shape == (S, 12 + 3 * L), (rig.dtype, rig.shape)
    out = dict(head_R=np.zeros((S, T, 3, 3), np.float32), head_t=np.zeros((S, T, 3), np.float32), reproj_rms=np.zeros((S, T), np.float32),
               valid=np.zeros((S, T), np.uint8), accepted=np.zeros((S, T), np.int64))
    out['head_R'][:] = np.eye(3, dtype=np.float32)
    for s in range(S):
        n = T if lengths is None else min(max(int(lengths[s]), 0), T)
        pose, dirty = None, False
        if state is not None and state[s, 12] != 0:
            pose = (state[s, :9].reshape(3, 3).copy(), state[s, 9:12].copy())
        if reset is not None and reset[s] != 0:
            pose, dirty = None, True
        for t in range(n):
            res = solve_frame(landmarks[s, t], rig[s], pose)
            dirty = True
            pose = (res['R'], res['t']) if res['valid'] else None
            out['valid'][s, t] = res['valid']
            out['accepted'][s, t] = res['accepted']
            if res['valid']:
                out['head_R'][s, t], out['head_t'][s, t], out['reproj_rms'][s, t] = pref.f32(res['R']), pref.f32(res['t']), pref.f32(res['rms'])
        if state is not None and dirty:
            state[s] = np.concatenate([I3.reshape(-1), np.zeros(4)]) if pose is None else np.concatenate([pose[0].reshape(-1), pose[1], [1.0]])
    return out


# ------------------------------------------------------------------------------------------------ eve_eye_pose_normalize_rt
def normalize_rt(rig, head_R, head_t, valid_in, out_hw):
    """The stages 2..6 of tests/eye_pose_ref.py continued from a float32 head_R [S, T, 3, 3] and head_t [S, T, 3]: rig float32
    [S, >= 12] (its first 12 entries are read), valid_in uint8 [S, T] or None -> eye_pose_ref.normalize's dict for N = S * T
    frames, valid ANDed with valid_in and with head_R and head_t being finite."""
    S, T = head_R.shape[:2]
    N = S * T
    rows = np.repeat(np.asarray(rig)[:, :12], T, axis=0)                      # [N, 12]
    head_R, head_t = np.ascontiguousarray(head_R).reshape(N, 3, 3), np.ascontiguousarray(head_t).reshape(N, 3)
    P = np.zeros((N, 18), dtype=np.float32)
    P[:, :4], P[:, 7:10], P[:, 10:16], P[:, 16:18] = rows[:, :4], head_t, rows[:, 4:10], rows[:, 10:12]
    res = pref.normalize(P, out_hw, head_R=head_R)
    ok = np.isfinite(head_R.reshape(N, 9)).all(axis=1)
    if valid_in is not None:
        ok = ok & (np.asarray(valid_in).reshape(N) != 0)
    bad = ~(res['valid'].astype(bool) & ok[None])
    res['valid'] = (~bad).astype(np.uint8)
    res['o'] = np.where(bad[..., None], np.float32(0), res['o'])
    res['h'] = np.where(bad[..., None], np.float32(0), res['h'])
    res['warp'] = np.where(bad[..., None, None], np.float32(0), res['warp'])
    res['R'] = np.where(bad[..., None, None], np.eye(3, dtype=np.float32), res['R'])
    return res


# ------------------------------------------------------------------------------------------------ stand-ins for FakeKernels
def face_pose_solve(self, landmarks, rig, lengths=None, state=None, reset=None):
    """Stand-in of HipKernels.face_pose_solve: `class Fakes(FakeKernels): face_pose_solve = ...`."""
    if not torch.is_tensor(landmarks) or landmarks.dtype != torch.float32 or landmarks.dim() != 4 or landmarks.shape[3] not in (2, 3):
        raise TypeError('face_pose_solve: landmarks must be float32 [S, T, L, 2 | 3]')
    S, T, L = landmarks.shape[:3]
    if not torch.is_tensor(rig) or rig.dtype != torch.float32 or tuple(rig.shape) != (S, 12 + 3 * L):
        raise TypeError('face_pose_solve: rig must be float32 [S, 12 + 3 L]')
    res = solve(landmarks.numpy(), rig.numpy(), None if lengths is None else lengths.numpy(), None if state is None else state.numpy(),
                None if reset is None else reset.numpy())
    return tuple(torch.from_numpy(res[k_]) for k_ in ('head_R', 'head_t', 'reproj_rms', 'valid'))


def eye_pose_normalize_rt(self, rig, head_R, head_t, valid_in, out_hw):
    """Stand-in of HipKernels.eye_pose_normalize_rt."""
    res = normalize_rt(rig.numpy(), head_R.numpy(), head_t.numpy(), None if valid_in is None else valid_in.numpy(),
                       (int(out_hw[0]), int(out_hw[1])))
    return tuple(torch.from_numpy(np.ascontiguousarray(res[k_])) for k_ in ('o', 'R', 'warp', 'h', 'valid'))
