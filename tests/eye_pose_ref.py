"""The contract of eve_eye_pose_normalize (include/eve_hip.h) in numpy, vectorised over the rows, the poses the tests share, and a
stand-in of HipKernels.eye_pose_normalize for the torch-CPU FakeKernels.

A pose row is 18 float32, widened to float64:
    (fx, fy, cx, cy,  r0, r1, r2,  t0, t1, t2,  l0, l1, l2,  q0, q1, q2,  focal_norm, distance_norm)
the camera matrix of the UNDISTORTED image, the head's rvec and tvec (cv2.solvePnP), the left and right eye centres in the head
model's coordinates (the length unit of t) and the virtual camera of the normalised patch: focal length f = focal_norm in patch
pixels, principal point (OW/2, OH/2), distance dn = distance_norm.  The procedure is the published one the reference cites (Zhang
et al. 2018, "Revisiting data normalization for appearance-based gaze estimation"); all arithmetic is float64, every operation
rounded on its own (numpy evaluates every ufunc on its own, so nothing is contracted here), in exactly this association:

 1. head_R        th = sqrt((r0*r0 + r1*r1) + r2*r2)
                  th == 0, or an r that is not finite: head_R = I.  Else k = r / th, c = cos(th), s = sin(th), v = 1.0 - c,
                  vk_i = v * k_i, sk_i = s * k_i and
                      head_R = [[c + vk0*k0,    vk0*k1 - sk2,  vk0*k2 + sk1],
                                [vk1*k0 + sk2,  c + vk1*k1,    vk1*k2 - sk0],
                                [vk2*k0 - sk1,  vk2*k1 + sk0,  c + vk2*k2  ]]
                  rounded to float32.  EVERY LATER STAGE CONTINUES FROM THE FLOAT32 VALUES JUST WRITTEN (H below).
 2. o_e           o_i = ((H[i][0]*c0 + H[i][1]*c1) + H[i][2]*c2) + t_i  with c the eye's centre; rounded to float32, continued from.
 3. R_e           d = sqrt((o0*o0 + o1*o1) + o2*o2), fw = o / d, hx = H[:, 0] (the head's x axis)
                  dn_ = cross(fw, hx), nd = sqrt((dn_0*dn_0 + dn_1*dn_1) + dn_2*dn_2), down = dn_ / nd
                  rt_ = cross(down, fw), nr likewise, right = rt_ / nr
                  cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
                  R_e = rows (right, down, fw), rounded to float32, continued from (R below).
 4. warp_e        = inv(W) = K . R^T . diag(1, 1, d / dn) . Kn^-1 in closed form: z = d / dn, g = 1.0 / f, px = (OW * 0.5) / f,
                  py = (OH * 0.5) / f,
                      A[i] = (R[0][i], R[1][i], R[2][i] * z)                                  (row i of R^T . diag)
                      B[0] = fx * A[0] + cx * A[2],  B[1] = fy * A[1] + cy * A[2],  B[2] = A[2]       (per column)
                      warp[i] = (B[i][0] * g,  B[i][1] * g,  (B[i][2] - B[i][0] * px) - B[i][1] * py)
                  rounded to float32 and NOT rescaled: its third row times a patch pixel is positive for a head in front of the
                  camera (fw_z * z at the patch centre), which eve_eye_warp_u8_* requires.
 5. h_e           m_i = (R[i][0]*H[0][2] + R[i][1]*H[1][2]) + R[i][2]*H[2][2]   (the third column of M = R_e . head_R)
                  h_e = (asin(min(max(m_1, -1.0), 1.0)), atan2(m_0, m_2)) as float32: (pitch, yaw) of the head's z axis in the
                  normalised camera.  (The clamp only matters where rounding carries m_1 past 1; asin would give a NaN there.)
 6. valid_e       every one of the 18 inputs finite  and  fx, fy, f, dn > 0  and  o_2 > 0  and  d > 0  and  nd > 0  and  nr > 0
                  (comparisons on the values above; a NaN fails them).  An invalid eye gets warp = 0 (a black patch), R = I,
                  o = 0, h = 0.  head_R does not depend on valid.

The layout is eye-major: o [2, N, 3], R [2, N, 3, 3], warp [2, N, 3, 3], h [2, N, 2], valid uint8 [2, N], left then right."""
import numpy as np
import torch

FIELDS = ('fx', 'fy', 'cx', 'cy', 'r0', 'r1', 'r2', 't0', 't1', 't2', 'l0', 'l1', 'l2', 'q0', 'q1', 'q2', 'focal_norm', 'distance_norm')
# the random poses of the issue: f = 140 on 96 x 128 frames, focal_norm = 220, distance_norm = 600
FRAME = (96, 128)             # (IH, IW)
CAMERA = (140.0, 140.0, 64.0, 48.0)
EYES = ((-32.0, -35.0, 25.0), (32.0, -35.0, 25.0))
FOCAL_NORM, DISTANCE_NORM = 220.0, 600.0


def pose_row(K=CAMERA, r=(0.0, 0.0, 0.0), t=(0.0, 0.0, 600.0), eyes=EYES, focal_norm=FOCAL_NORM, distance_norm=DISTANCE_NORM):
    return np.array(list(K) + list(r) + list(t) + list(eyes[0]) + list(eyes[1]) + [focal_norm, distance_norm], dtype=np.float32)


def random_poses(n, seed):
    """rvec in [-0.5, 0.5]^3, t in (+-60, +-40, 450..750), the eye centres (-+32, -35, 25) -> float32 [n, 18]."""
    g = np.random.default_rng(seed)
    rows = [pose_row(r=g.uniform(-0.5, 0.5, 3), t=(g.uniform(-60, 60), g.uniform(-40, 40), g.uniform(450, 750))) for _ in range(n)]
    return np.stack(rows)


def along_head_axis(r, axis, scale=512.0):
    """A plain float32 row whose eye origins lie EXACTLY along column `axis` of its own float32 head_R: zero eye centres and
    t = scale * head_R[:, axis], a power of two times float32 values and so exact.  (head_R as this file evaluates it; a device
    whose head_R sits an ulp away sees an origin a hair off the axis, hence the candidates below come in handfuls.)"""
    H = f32(rodrigues(np.array([r], dtype=np.float32).astype(np.float64)))[0]
    return pose_row(r=r, t=tuple(scale * H[:, axis]), eyes=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))


# rvecs whose along_head_axis(r, 0) rows this contract marks INVALID with finite inputs, o_z > 0 and d > 0: forward is parallel to
# the head's x axis and both cross products vanish exactly (about six in ten rows built this way do; the others leave rounding
# residue in the cross product and are valid)
PARALLEL_RVECS = ((0.0, -1.2623804807662964, 0.0), (0.0, -1.2623804807662964, 0.0, 1024.0),
                  (0.3461553454399109, -0.3489673435688019, 1.4916298389434814),
                  (-0.2863444685935974, -0.9044608473777771, -1.2277408838272095),
                  (-1.4149038791656494, 0.6576592922210693, -1.4520248174667358))
# rvecs whose along_head_axis(r, 1) rows are VALID with |m_1| > 1 by rounding alone (down is the head's -z axis): without the
# clamp of stage 5 asin would return a NaN for them; with it h = (-pi/2, 0)
CLAMP_RVECS = ((0.8604759573936462, 0.0, 0.0), (0.9265064597129822, 0.0, 0.0), (0.8526114821434021, 0.0, 0.0))


def parallel_rows():
    return [along_head_axis(r[:3], 0, *r[3:]) for r in PARALLEL_RVECS]


def clamp_rows():
    return [along_head_axis(r, 1) for r in CLAMP_RVECS]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def norm3(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def rodrigues(r):
    """r float64 [N, 3] -> head_R float64 [N, 3, 3], not yet rounded to float32 (stage 1)."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(all='ignore'):
        th = norm3(r)
        ok = np.isfinite(r).all(axis=1) & (th != 0)
        k = r / np.where(ok, th, 1.0)[:, None]
        c, s = np.cos(th), np.sin(th)
        v = 1.0 - c
        vk, sk = v[:, None] * k, s[:, None] * k
        k0, k1, k2 = k[:, 0], k[:, 1], k[:, 2]
        R = np.stack([np.stack([c + vk[:, 0] * k0, vk[:, 0] * k1 - sk[:, 2], vk[:, 0] * k2 + sk[:, 1]], axis=-1),
                      np.stack([vk[:, 1] * k0 + sk[:, 2], c + vk[:, 1] * k1, vk[:, 1] * k2 - sk[:, 0]], axis=-1),
                      np.stack([vk[:, 2] * k0 - sk[:, 1], vk[:, 2] * k1 + sk[:, 0], c + vk[:, 2] * k2], axis=-1)], axis=-2)
    return np.where(ok[:, None, None], R, np.eye(3))


def f32(a):
    with np.errstate(all='ignore'):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


def eye_rotation(o, H):
    """Stage 3: o float64 [N, 3], H float64 [N, 3, 3] -> (R float64 [N, 3, 3] with rows right, down, forward; d, nd, nr [N])."""
    with np.errstate(all='ignore'):
        d = norm3(o)
        fw = o / d[:, None]
        dn_ = cross(fw, H[:, :, 0])
        nd = norm3(dn_)
        down = dn_ / nd[:, None]
        rt_ = cross(down, fw)
        nr = norm3(rt_)
        right = rt_ / nr[:, None]
    return np.stack([right, down, fw], axis=-2), d, nd, nr


def inverse_warp(R, d, K, f, dn, out_hw):
    """Stage 4: R float64 [N, 3, 3], d [N], K = (fx, fy, cx, cy) each [N], f, dn [N] -> inv(W) float64 [N, 3, 3], not rounded."""
    fx, fy, cx, cy = K
    OH, OW = out_hw
    with np.errstate(all='ignore'):
        z, g, px, py = d / dn, 1.0 / f, (OW * 0.5) / f, (OH * 0.5) / f
        A = np.stack([R[:, 0, :], R[:, 1, :], R[:, 2, :] * z[:, None]], axis=-1)          # A[n][i][j]
        B = np.stack([fx[:, None] * A[:, 0] + cx[:, None] * A[:, 2], fy[:, None] * A[:, 1] + cy[:, None] * A[:, 2], A[:, 2]], axis=-2)
        return np.stack([B[:, :, 0] * g[:, None], B[:, :, 1] * g[:, None],
                         (B[:, :, 2] - B[:, :, 0] * px[:, None]) - B[:, :, 1] * py[:, None]], axis=-1)


def normalize(pose, out_hw, head_R=None):
    """pose float32 [N, 18], out_hw = (OH, OW) -> dict of the contract's outputs (head_R [N,3,3], o [2,N,3], R [2,N,3,3], warp
    [2,N,3,3], h [2,N,2] float32, valid uint8 [2,N]) and, for the cross-checks, float64 values before their rounding to float32
    (head_R64 [N,3,3]; o64 [2,N,3], R64 [2,N,3,3], m64 [2,N,3], d [2,N]; garbage where the eye is invalid).  head_R: float32
    [N, 3, 3] to evaluate the stages 2..6 from instead of stage 1's own result (a device's head_R, which may sit one float32 ulp
    away)."""
    pose = np.asarray(pose)
    assert pose.dtype == np.float32 and pose.ndim == 2 and pose.shape[1] == 18, (pose.dtype, pose.shape)
    out_hw = (int(out_hw[0]), int(out_hw[1]))
    N = pose.shape[0]
    p = pose.astype(np.float64)
    K, t, f, dn = (p[:, 0], p[:, 1], p[:, 2], p[:, 3]), p[:, 7:10], p[:, 16], p[:, 17]
    head_R64 = rodrigues(p[:, 4:7])
    if head_R is None:
        head_R = f32(head_R64)
    else:
        head_R = np.asarray(head_R)
        assert head_R.dtype == np.float32 and head_R.shape == (N, 3, 3)
    H = head_R.astype(np.float64)
    row_ok = np.isfinite(p).all(axis=1) & (K[0] > 0) & (K[1] > 0) & (f > 0) & (dn > 0)
    out = {k_: [] for k_ in ('o', 'R', 'warp', 'h', 'valid', 'o64', 'R64', 'm64', 'd')}
    with np.errstate(all='ignore'):
        for e in range(2):
            c = p[:, 10 + 3 * e:13 + 3 * e]
            o64 = ((H[:, :, 0] * c[:, 0:1] + H[:, :, 1] * c[:, 1:2]) + H[:, :, 2] * c[:, 2:3]) + t
            o32 = f32(o64)
            o = o32.astype(np.float64)
            R64, d, nd, nr = eye_rotation(o, H)
            R32 = f32(R64)
            R = R32.astype(np.float64)
            warp32 = f32(inverse_warp(R, d, K, f, dn, out_hw))
            m = (R[:, :, 0] * H[:, 0:1, 2] + R[:, :, 1] * H[:, 1:2, 2]) + R[:, :, 2] * H[:, 2:3, 2]
            h64 = np.stack([np.arcsin(np.minimum(np.maximum(m[:, 1], -1.0), 1.0)), np.arctan2(m[:, 0], m[:, 2])], axis=-1)
            valid = row_ok & (o[:, 2] > 0) & (d > 0) & (nd > 0) & (nr > 0)
            v1, v2 = valid[:, None], valid[:, None, None]
            out['o'].append(np.where(v1, o32, np.float32(0)))
            out['R'].append(np.where(v2, R32, np.eye(3, dtype=np.float32)))
            out['warp'].append(np.where(v2, warp32, np.float32(0)))
            out['h'].append(np.where(v1, f32(h64), np.float32(0)))
            out['valid'].append(valid.astype(np.uint8))
            for k_, a in (('o64', o64), ('R64', R64), ('m64', m), ('d', d)):
                out[k_].append(a)
    out = {k_: np.stack(v) for k_, v in out.items()}
    for k_ in ('o', 'R', 'warp', 'h'):
        assert out[k_].dtype == np.float32
    out['head_R'], out['head_R64'] = head_R, head_R64
    return out


def patch_corners_inside(res, frame_hw, out_hw):
    """The four corners of every valid eye's patch through its warp: (all inside the frame, all with Wd > 0)."""
    (IH, IW), (OH, OW) = frame_hw, out_hw
    corners = np.array([[0, 0, 1], [OW - 1, 0, 1], [0, OH - 1, 1], [OW - 1, OH - 1, 1]], dtype=np.float64)
    q = np.einsum('enij,cj->enci', res['warp'].astype(np.float64), corners)
    u, v, w = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2], q[..., 2]
    return bool(((u >= 0) & (u <= IW - 1) & (v >= 0) & (v <= IH - 1)).all()), bool((w > 0).all())


# ------------------------------------------------------------------------------------------------ stand-in for FakeKernels
def eye_pose_normalize(self, pose, out_hw):
    """Stand-in of HipKernels.eye_pose_normalize: `class Fakes(FakeKernels): eye_pose_normalize = ...`."""
    if not torch.is_tensor(pose) or pose.dtype != torch.float32 or pose.dim() != 2 or pose.shape[1] != 18:
        raise TypeError('eye_pose_normalize: pose must be float32 [N, 18]')
    res = normalize(pose.numpy(), (int(out_hw[0]), int(out_hw[1])))
    return tuple(torch.from_numpy(np.ascontiguousarray(res[k_])) for k_ in ('head_R', 'o', 'R', 'warp', 'h', 'valid'))
