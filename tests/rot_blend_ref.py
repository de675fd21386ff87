"""float64 numpy restatement of dense inference's blend in rotation space (the recipe in include/mmego_hip.h: mmego_blend_rot), written
frame by frame and bone by bone with plain loops and by ANOTHER METHOD than the kernel's: the mean rotation of a bone is taken from the
singular value decomposition of the weighted sum S (U diag(1, 1, det(U V^T)) V^T, the proper rotation nearest S) and turned into a
quaternion by Shepperd's branches, where the kernel takes the top eigenvector of a 4 x 4 matrix by Jacobi sweeps; the gap between the
two largest eigenvalues of that matrix is, in singular values s1 >= s2 >= s3 of S and d = sign(det S), 2 (s2 + d s3).  A helper for
tests/test_rot_blend_cpu.py, test_rot_blend_gpu.py and test_dense_rot_gpu.py; the maker of rigid test rows with their rotations lives
here too."""
import numpy as np

from bone_blend_ref import LOWER_WALK, UPPER_WALK, random_rotations          # noqa: F401  (the walk tables, spelled out by hand there)

ROT_UPPER = tuple(c for c, _ in UPPER_WALK)          # Upper_Net's rotation of a bone: the child's slot
ROT_LOWER = (0, 1, 2, 3, 4, 5)
TINY = 1e-9


def canonical(q):
    """The quaternion (w, x, y, z) with its first non-zero component positive (rows of an array alike)."""
    q = np.array(q, dtype=np.float64)
    flat = q.reshape(-1, 4)
    for v in flat:
        nz = np.flatnonzero(v)
        if len(nz) and v[nz[0]] < 0:
            v *= -1.0
    return flat.reshape(q.shape)


def nearest_rotation(S):
    """-> (the proper rotation Q that maximises tr(Q^T S), the gap lambda_1 - lambda_2 of the quaternion problem's 4 x 4 matrix)."""
    U, s, Vt = np.linalg.svd(S)
    d = 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0
    return U @ np.diag([1.0, 1.0, d]) @ Vt, 2.0 * (s[1] + d * s[2])


def quaternion(R):
    """(w, x, y, z) of a rotation matrix, canonical sign: Shepperd's method, the branch of the largest of (trace, R11, R22, R33)."""
    t = np.trace(R)
    k = int(np.argmax([t, R[0, 0], R[1, 1], R[2, 2]]))
    if k == 0:
        q = np.array([1.0 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + 2.0 * R[0, 0] - t, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2.0 * R[1, 1] - t, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2.0 * R[2, 2] - t])
    q = q / np.sqrt((q * q).sum())
    q[np.abs(q) < 1e-300] = 0.0
    return canonical(q)


def matrix(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def angle(D):
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.sqrt((v * v).sum()), 0.5 * (np.trace(D) - 1.0)))


def blend_rot(src, q, Rh, off, row, w, bones, rot_idx, body, min_gap=None):
    """-> (dst [F, 3 J], quat [F, NB, 4], spread [F], rot_spread [F] float64, fallback [F] int) of mmego_blend_rot; entries whose row is
    outside src are skipped.  min_gap (a list): receives (lambda_1 - lambda_2) / W of every bone of every frame with a cover."""
    src = np.asarray(src, dtype=np.float64)
    nrows, J = src.shape[0], src.shape[1] // 3
    q = np.asarray(q, dtype=np.float64).reshape(nrows, -1, 3, 3)
    Rh = np.asarray(Rh, dtype=np.float64).reshape(nrows, 3, 3)
    body = np.asarray(body, dtype=np.float64).reshape(-1, 3)
    F, NB = len(off) - 1, len(bones)
    dst, quat, spr, rspr, fb = np.zeros((F, 3 * J)), np.zeros((F, NB, 4)), np.zeros(F), np.zeros(F), np.zeros(F, dtype=np.int64)
    children = [c for c, _ in bones]
    for f in range(F):
        ks = [k for k in range(int(off[f]), int(off[f + 1])) if 0 <= int(row[k]) < nrows]
        wk = [float(w[k]) for k in ks]
        W = 0.0
        for v in wk:
            W += v
        if not ks or W == 0.0:
            continue
        rows = [int(row[k]) for k in ks]
        x = [src[r].reshape(J, 3) for r in rows]
        Qbar = []
        for b in range(NB):
            A = [Rh[r].T @ q[r, rot_idx[b]] for r in rows]
            S = np.zeros((3, 3))
            for v, a in zip(wk, A):
                S += v * a
            Q, gap = nearest_rotation(S)
            if min_gap is not None:
                min_gap.append(gap / W)
            if gap <= TINY * W:
                fb[f] += 1
                Q, _ = nearest_rotation(A[int(np.argmax(wk))])          # (numpy's argmax: the first of equal maxima)
            quat[f, b] = quaternion(Q)
            Qbar.append((Q, A))
        pos = np.zeros((J, 3))
        if len(ks) == 1:
            pos[:] = x[0]
        else:
            for j in range(J):
                if j not in children:
                    acc = np.zeros(3)
                    for v, xk in zip(wk, x):
                        acc += v * xk[j]
                    pos[j] = acc / W
            for b, (c, p) in enumerate(bones):
                pos[c] = pos[p] + Qbar[b][0] @ body[b]
            tot = 0.0
            for Q, A in Qbar:
                for v, a in zip(wk, A):
                    tot += v * angle(Q.T @ a) ** 2
            rspr[f] = np.sqrt(tot / (NB * W)) if tot > 0.0 else 0.0
        dst[f] = pos.ravel()
        tot = 0.0
        for v, xk in zip(wk, x):
            tot += v * ((xk - pos) ** 2).sum()
        spr[f] = np.sqrt(tot / (J * W)) if tot > 0.0 else 0.0
    return dst, quat, spr, rspr, fb


def fk_from_quaternions(roots, quat, bones, body):
    """Positions [n, J, 3] from root positions (roots [n, J, 3]: only the rows of joints that are no bone's child are read), the
    quaternions quat [n, NB, 4] and the rest bones body [NB, 3]: pos_c = pos_p + R(quat_b) body_b, bones in their listed order."""
    pos = np.array(roots, dtype=np.float64)
    body = np.asarray(body, dtype=np.float64)
    for i in range(len(pos)):
        for b, (c, p) in enumerate(bones):
            pos[i, c] = pos[i, p] + matrix(quat[i, b]) @ body[b]
    return pos


def rigid_rows(rng, n, J, bones, rot_idx, NQ, body, root_range=3.0, max_angle=0.5):
    """n window rows as the nets make them, for which the GPU tests' bounds hold: per bone a random base rotation G_b, the same in every
    row, times a perturbation P of at most max_angle radians about a random axis -- the WORLD rotation of the bone in that row; per row a
    random proper head rotation Rh (a column flipped where the determinant is negative) and q = Rh G_b P, so that Rh^T q is the world
    rotation again; the roots uniform within root_range metres, the joints by forward kinematics in the world frame.  Everything in
    float64 with one float32 rounding.  -> (src [n, 3 J], q [n, NQ, 9], Rh [n, 9]) float32; rotations no bone names are the identity."""
    body = np.asarray(body, dtype=np.float64)
    base = random_rotations(rng, len(bones))
    for G in base:
        if np.linalg.det(G) < 0:
            G[:, 0] *= -1.0
    src, q, Rh = np.zeros((n, J, 3)), np.tile(np.eye(3), (n, NQ, 1, 1)), np.zeros((n, 3, 3))
    children = [c for c, _ in bones]
    for r in range(n):
        H = random_rotations(rng, 1)[0]
        if np.linalg.det(H) < 0:
            H[:, 0] *= -1.0
        Rh[r] = H
        for j in range(J):
            if j not in children:
                src[r, j] = rng.uniform(-root_range, root_range, 3)
        for b, (c, p) in enumerate(bones):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            a = rng.uniform(-max_angle, max_angle)
            K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
            P = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
            A = base[b] @ P
            q[r, rot_idx[b]] = H @ A
            src[r, c] = src[r, p] + A @ body[b]
    return src.reshape(n, 3 * J).astype(np.float32), q.reshape(n, NQ, 9).astype(np.float32), Rh.reshape(n, 9).astype(np.float32)
