"""float64 numpy restatement of dense inference's temporal filter in rotation space (the recipe in include/mmego_hip.h:
mmego_smooth_rot), frame by frame and by ANOTHER ROUTE than the kernel's: the coefficients come from smooth_ref.coefficients (a
least-squares solve, not the moment matrix's cofactors), the filtered rotation of a bone is the top eigenvector that numpy.linalg.eigh
finds for the symmetric 4 x 4 matrix of S = sum_k c_k A_k, batched over the bones (the kernel runs Jacobi sweeps per lane), and the
forward kinematics are plain loops.  A helper for tests/test_rot_smooth_cpu.py, test_smooth_rot_gpu.py and test_dense_rot_smooth_gpu.py;
the maker of the GPU tests' rigid rows with their quaternions lives here too."""
import numpy as np

import rot_blend_ref as rref
import smooth_ref as sref

TINY = 1e-9


def matrices(quat):
    """Rotation matrices [..., 3, 3] of quaternions [..., 4] (w, x, y, z), by the recipe's formula (1 - 2 (y^2 + z^2) on the diagonal:
    a quaternion that is unit only up to rounding gives what the kernel's br_matrix gives)."""
    q = np.asarray(quat, dtype=np.float64)
    w, x, y, z = (q[..., i] for i in range(4))
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def quat_matrix(S):
    """The symmetric 4 x 4 matrices [..., 4, 4] whose top eigenvector is the quaternion of the rotation nearest S [..., 3, 3]."""
    S = np.asarray(S, dtype=np.float64)
    N = np.empty(S.shape[:-2] + (4, 4))
    s = lambda i, j: S[..., i, j]
    N[..., 0, 0] = s(0, 0) + s(1, 1) + s(2, 2)
    N[..., 1, 1] = s(0, 0) - s(1, 1) - s(2, 2)
    N[..., 2, 2] = -s(0, 0) + s(1, 1) - s(2, 2)
    N[..., 3, 3] = -s(0, 0) - s(1, 1) + s(2, 2)
    N[..., 0, 1] = N[..., 1, 0] = s(2, 1) - s(1, 2)
    N[..., 0, 2] = N[..., 2, 0] = s(0, 2) - s(2, 0)
    N[..., 0, 3] = N[..., 3, 0] = s(1, 0) - s(0, 1)
    N[..., 1, 2] = N[..., 2, 1] = s(0, 1) + s(1, 0)
    N[..., 1, 3] = N[..., 3, 1] = s(0, 2) + s(2, 0)
    N[..., 2, 3] = N[..., 3, 2] = s(1, 2) + s(2, 1)
    return N


def nearest(S):
    """-> (canonical unit quaternions [..., 4] of the proper rotations nearest S [..., 3, 3], the gaps lambda_1 - lambda_2 [...])."""
    lam, vec = np.linalg.eigh(quat_matrix(S))
    q = vec[..., :, 3]
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    q[np.abs(q) < 1e-300] = 0.0
    return rref.canonical(q), lam[..., 3] - lam[..., 2]


def smooth_rot(src, quat, seg, w, D, bones, body, min_gap=None, sum_abs=None):
    """-> (dst [F, 3 J], quat_out [F, NB, 4], moved [F], rot_moved [F] float64, fallback [F] int) of mmego_smooth_rot.  min_gap, sum_abs
    (lists): receive every filtered frame's least (lambda_1 - lambda_2) / sum |c_k| over its bones, and its sum |c_k|."""
    src = np.asarray(src, dtype=np.float64)
    quat = np.asarray(quat, dtype=np.float64)
    body = np.asarray(body, dtype=np.float64).reshape(-1, 3)
    F, J, NB, H = src.shape[0], src.shape[1] // 3, len(bones), len(w) // 2
    A = matrices(quat)                                                   # [F, NB, 3, 3]
    dst, qout, moved, rmoved, fb = src.copy(), quat.copy(), np.zeros(F), np.zeros(F), np.zeros(F, dtype=np.int64)
    children = [c for c, _ in bones]
    coefs = {}
    for f in range(F):
        taps = sref.valid_taps(seg, f, H)
        if len(taps) <= 1:
            continue
        key = tuple(taps)
        if key not in coefs:
            coefs[key] = sref.coefficients(w, taps, D)
        ck = coefs[key]
        W = float(np.abs(ck).sum())
        rows = f + np.asarray(taps)
        S = np.einsum("k,kbij->bij", ck, A[rows])
        q, gap = nearest(S)
        if min_gap is not None:
            min_gap.append(float(gap.min()) / W)
        if sum_abs is not None:
            sum_abs.append(W)
        fell = ~(gap > TINY * W)
        if fell.any():
            q[fell] = nearest(A[f][fell])[0]
            fb[f] = int(fell.sum())
        Q = matrices(q)
        x = src[rows].reshape(len(taps), J, 3)
        pos = np.zeros((J, 3))
        for j in range(J):
            if j not in children:
                for c, xk in zip(ck, x):
                    pos[j] += c * xk[j]
        tot = 0.0
        for b, (c, p) in enumerate(bones):
            pos[c] = pos[p] + Q[b] @ body[b]
            tot += rref.angle(Q[b].T @ A[f, b]) ** 2
        dst[f], qout[f] = pos.ravel(), q
        moved[f] = np.sqrt(((pos - src[f].reshape(J, 3)) ** 2).sum() / J)
        rmoved[f] = np.sqrt(tot / NB) if tot > 0.0 else 0.0
    return dst, qout, moved, rmoved, fb


def axis_angle(axis, angle):
    """The rotation matrix of ``angle`` radians about ``axis`` (Rodrigues)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rows_of(rng, rot, bones, body, J, signs=True, root_sigma=0.7, roots=None):
    """Rigid rows for world rotations rot [F, NB, 3, 3] (float64): roots N(0, root_sigma) per frame (or ``roots`` [F, J, 3]), the joints
    by forward kinematics over ``bones``, the quaternions by Shepperd's branches with a random sign each (``signs``), everything
    rounded once.  -> (src [F, 3 J] float32, quat [F, NB, 4] float32, the exact positions [F, 3 J] and quaternions [F, NB, 4], float64,
    canonical sign)."""
    F, NB = rot.shape[:2]
    body = np.asarray(body, dtype=np.float64)
    pos = rng.normal(0.0, root_sigma, (F, J, 3)) if roots is None else np.array(roots, dtype=np.float64)
    q = np.zeros((F, NB, 4))
    for f in range(F):
        for b, (c, p) in enumerate(bones):
            pos[f, c] = pos[f, p] + rot[f, b] @ body[b]
            q[f, b] = rref.quaternion(rot[f, b])
    sign = np.where(rng.random((F, NB, 1)) < 0.5, -1.0, 1.0) if signs else 1.0
    return pos.reshape(F, 3 * J).astype(np.float32), (q * sign).astype(np.float32), pos.reshape(F, 3 * J), q


def jittery_rotations(rng, F, NB, max_angle=0.6):
    """rot [F, NB, 3, 3]: per bone a random base rotation times, in every frame, a rotation of at most max_angle radians about a random
    axis."""
    base = rref.random_rotations(rng, NB)
    for G in base:
        if np.linalg.det(G) < 0:
            G[:, 0] *= -1.0
    rot = np.zeros((F, NB, 3, 3))
    for f in range(F):
        for b in range(NB):
            rot[f, b] = base[b] @ axis_angle(rng.normal(size=3), rng.uniform(-max_angle, max_angle))
    return rot
