"""Float64 yardstick of the aligned evaluation metrics (mmego_pose_errors_aligned, mmego_pose_accel_errors; csrc/metrics.hip).

The alignment is the SVD solution (Umeyama, IEEE PAMI 13(4), 1991) with its determinant correction: of the kernel's method -- Horn's
quaternion form with a Jacobi eigen-solve -- it shares only the definition.  `horn_fit` is a second, independent formulation (the
quaternion form through numpy.linalg.eigh) that tests/test_pose_metrics_cpu.py holds the yardstick itself against.  numpy only."""
import numpy as np

UPPER_MAP = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 20]
LOWER_MAP = [12, 13, 14, 15, 16, 17, 18, 19]


def assemble(upper, lower, target):
    """(p, g) float64 [..., J, 3]: the J joints the kernels compare.  lower given: the 21-joint skeleton (lower overwrites the shared
    hips) against the target; lower None: the 15 upper joints against target[..., UPPER_MAP, :]."""
    upper, target = np.asarray(upper, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if lower is None:
        return upper, target[..., UPPER_MAP, :]
    p = np.zeros(upper.shape[:-2] + (21, 3))
    p[..., UPPER_MAP, :] = upper
    p[..., LOWER_MAP, :] = np.asarray(lower, dtype=np.float64)
    return p, target


def _centred(p, g):
    pb, gb = p.mean(axis=-2, keepdims=True), g.mean(axis=-2, keepdims=True)
    return p - pb, g - gb, pb[..., 0, :], gb[..., 0, :]


def _angle_deg(R):
    """Rotation angle in [0, 180] from sin (the skew part) and cos (the trace): well conditioned at both ends."""
    v = 0.5 * np.stack((R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]), axis=-1)
    return np.degrees(np.arctan2(np.linalg.norm(v, axis=-1), 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)))


def umeyama_fit(p, g):
    """p, g [F, J, 3] -> (R [F,3,3] proper rotations, s [F]) minimising sum_j |s R (p_j - pbar) + gbar - g_j|^2.  R is the optimum for
    s = 1 as well.  A zero covariance gives R = I; a prediction without spread s = 0."""
    pc, gc, _, _ = _centred(p, g)
    C = np.einsum("fja,fjb->fab", gc, pc)                       # target x prediction^T
    U, D, Vt = np.linalg.svd(C)
    sign = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    sign[sign == 0] = 1.0
    S = np.ones_like(D)
    S[:, 2] = sign                                               # the determinant correction: never a reflection
    R = np.einsum("fab,fb,fbc->fac", U, S, Vt)
    zero = ~np.any(C != 0.0, axis=(1, 2))
    R[zero] = np.eye(3)
    pp = np.sum(pc * pc, axis=(1, 2))
    s = np.where(pp > 0.0, np.sum(D * S, axis=1) / np.where(pp > 0.0, pp, 1.0), 0.0)
    return R, s


def horn_fit(p, g):
    """The same optimum through Horn's quaternion form and numpy.linalg.eigh (second formulation)."""
    pc, gc, _, _ = _centred(p, g)
    S = np.einsum("fja,fjb->fab", pc, gc)
    N = np.empty(S.shape[:1] + (4, 4))
    xx, yy, zz = S[:, 0, 0], S[:, 1, 1], S[:, 2, 2]
    N[:, 0, 0], N[:, 1, 1], N[:, 2, 2], N[:, 3, 3] = xx + yy + zz, xx - yy - zz, -xx + yy - zz, -xx - yy + zz
    N[:, 0, 1] = N[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
    N[:, 1, 2] = N[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]
    N[:, 2, 3] = N[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
    lam, vec = np.linalg.eigh(N)
    q = vec[:, :, 3]
    zero = ~np.any(S != 0.0, axis=(1, 2))
    q[zero] = (1.0, 0.0, 0.0, 0.0)
    w, x, y, z = q.T
    R = np.stack((np.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)), -1),
                  np.stack((2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)), -1),
                  np.stack((2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1)), 1)
    pp = np.sum(pc * pc, axis=(1, 2))
    s = np.where(pp > 0.0, lam[:, 3] / np.where(pp > 0.0, pp, 1.0), 0.0)
    return R, s


def fit_errors(p, g, fit=umeyama_fit):
    """-> (rigid [F, J], similarity [F, J], angle_deg [F], shift [F], s [F])."""
    pc, gc, pb, gb = _centred(p, g)
    R, s = fit(p, g)
    rp = np.einsum("fab,fjb->fja", R, pc)
    return (np.linalg.norm(rp - gc, axis=-1), np.linalg.norm(s[:, None, None] * rp - gc, axis=-1), _angle_deg(R),
            np.linalg.norm(pb - gb, axis=-1), s)


def root_relative(p, g):
    return np.linalg.norm((p - p[..., :1, :]) - (g - g[..., :1, :]), axis=-1)


def joint_errors(p, g):
    return np.linalg.norm(p - g, axis=-1)


def pck(p, g, thr):
    """[F, len(thr)]: fraction of the J joints whose absolute error is <= thr[k]."""
    e = joint_errors(p, g)
    return np.stack([(e <= float(t)).mean(axis=-1) for t in thr] or [np.zeros(e.shape[:-1])], axis=-1)[..., :len(thr)]


def aligned_rows(upper, lower, target, thr=()):
    """The rows of mmego_pose_errors_aligned, float64 [F, 3 J + 3 + len(thr)]."""
    p, g = assemble(upper, lower, target)
    p, g = p.reshape(-1, p.shape[-2], 3), g.reshape(-1, g.shape[-2], 3)
    rigid, sim, ang, shift, s = fit_errors(p, g)
    return np.concatenate((root_relative(p, g), rigid, sim, ang[:, None], shift[:, None], s[:, None], pck(p, g, thr)), axis=1)


def accel_errors(upper, lower, target):
    """mmego_pose_accel_errors: [B, T, ...] inputs -> [B, J], mean over t = 1 .. T-2 of the error of the second differences."""
    p, g = assemble(upper, lower, target)
    acc = lambda a: a[:, :-2] - 2.0 * a[:, 1:-1] + a[:, 2:]
    return np.linalg.norm(acc(p) - acc(g), axis=-1).mean(axis=1)


# ---- test inputs: fp32 skeletons of the kinds the tests name --------------------------------------------------------------------------
def random_rotations(rng, n):
    """-> (R [n,3,3] proper rotations about random axes, their angles in degrees, uniform in [0, 180])."""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0.0, np.pi, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3) + np.sin(ang)[:, None, None] * K + (1.0 - np.cos(ang))[:, None, None] * (K @ K)
    return R, np.degrees(ang)


def similarity(rng, x, scale=True, shift=1.0):
    """x [F, J, 3] through one random similarity (scale 0.5-2, proper rotation, shift of that spread) per frame -> (y float64, angle_deg)."""
    F = x.shape[0]
    R, ang = random_rotations(rng, F)
    s = rng.uniform(0.5, 2.0, F) if scale else np.ones(F)
    return s[:, None, None] * np.einsum("fab,fjb->fja", R, x) + rng.normal(0.0, shift, (F, 1, 3)), ang


def make_frames(kind, rng, F):
    """-> (pred21 [F,21,3] fp32, target [F,21,3] fp32, known fit angle in degrees or None).  Kinds: noisy, mirrored, similar,
    identical, collinear (the prediction on a line), pred_point, target_point (all joints of one of them on one point)."""
    g = (rng.normal(0.0, 0.4, (F, 21, 3)) + np.array([0.8, 0.0, 0.2])).astype(np.float32)
    ang = None
    if kind == "noisy":
        p = g + rng.normal(0.0, 0.05, g.shape)
    elif kind == "mirrored":
        p = g * np.array([-1.0, 1.0, 1.0]) + rng.normal(0.0, 0.05, g.shape)
    elif kind == "similar":
        p, ang = similarity(rng, g.astype(np.float64))
    elif kind == "identical":
        p = g.copy()
    elif kind == "collinear":
        p = rng.normal(size=(F, 1, 3)) + rng.normal(size=(F, 21, 1)) * rng.normal(size=(F, 1, 3))
    elif kind == "pred_point":
        p = np.repeat(rng.normal(size=(F, 1, 3)), 21, axis=1)
    elif kind == "target_point":
        p = g + rng.normal(0.0, 0.05, g.shape)
        g = np.repeat(g[:, :1], 21, axis=1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, dtype=np.float32), g, ang


def split(pred21, J):
    """pred21 [..., 21, 3] -> (upper [..., 15, 3], lower [..., 8, 3] or None for J = 15), contiguous."""
    return np.ascontiguousarray(pred21[..., UPPER_MAP, :]), (np.ascontiguousarray(pred21[..., LOWER_MAP, :]) if J == 21 else None)
