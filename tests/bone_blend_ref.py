"""float64 numpy restatement of the bone-length-preserving blend and of the bone-length table (the recipes in include/mmego_hip.h:
mmego_blend_bones, mmego_bone_length_dev), written frame by frame and bone by bone with plain loops -- another route than the
lane-per-joint kernel with its wave shuffles.  A helper for tests/test_bone_blend_gpu.py and tests/test_dense_bones_gpu.py; the makers
of rigid test rows live here too."""
import numpy as np

UPPER_WALK = ((3, 14), (2, 3), (1, 2), (4, 2), (8, 2), (5, 4), (6, 5), (7, 6), (9, 8), (10, 9), (11, 10), (0, 1), (12, 0), (13, 0))
LOWER_WALK = ((1, 0), (2, 1), (3, 2), (5, 4), (6, 5), (7, 6))
TINY = 1e-9


def blend_bones(src, off, row, w, bones, bone_len):
    """-> (dst [F, 3 J] float64, spread [F] float64, fallback [F] int) of mmego_blend_bones; entries whose row is outside src are skipped."""
    src = np.asarray(src, dtype=np.float64)
    nrows, J = src.shape[0], src.shape[1] // 3
    F = len(off) - 1
    dst, spr, fb = np.zeros((F, 3 * J)), np.zeros(F), np.zeros(F, dtype=np.int64)
    children = [c for c, _ in bones]
    for f in range(F):
        ks = [k for k in range(int(off[f]), int(off[f + 1])) if 0 <= int(row[k]) < nrows]
        wk = [float(w[k]) for k in ks]
        W = 0.0
        for v in wk:
            W += v
        if not ks or W == 0.0:
            continue
        x = [src[int(row[k])].reshape(J, 3) for k in ks]
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
            for (c, p), L in zip(bones, bone_len):
                L = float(L)
                s = np.zeros(3)
                for v, xk in zip(wk, x):
                    s += v * (xk[c] - xk[p])
                n = np.sqrt((s * s).sum())
                if n > TINY * W * L and n > 0.0:
                    u = s / n
                else:
                    fb[f] += 1
                    first = int(np.argmax(wk))                       # (numpy's argmax: the first of equal maxima)
                    d = x[first][c] - x[first][p]
                    m = np.sqrt((d * d).sum())
                    u = d / m if m > 0.0 else np.zeros(3)
                pos[c] = pos[p] + L * u
        dst[f] = pos.ravel()
        tot = 0.0
        for v, xk in zip(wk, x):
            tot += v * ((xk - pos) ** 2).sum()
        spr[f] = np.sqrt(tot / (J * W)) if tot > 0.0 else 0.0
    return dst, spr, fb


def bone_length_dev(X, bones, bone_len):
    """-> [n, NB] float64: | |X[r, c] - X[r, p]| - L |."""
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(len(X), -1, 3)
    out = np.zeros((len(X), len(bones)))
    for b, ((c, p), L) in enumerate(zip(bones, bone_len)):
        for r in range(len(X)):
            d = X[r, c] - X[r, p]
            out[r, b] = abs(np.sqrt((d * d).sum()) - float(L))
    return out


def bone_lengths(X, bones):
    """-> [n, NB] float64 lengths of the bones of the rows X [n, 3 J]."""
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(len(X), -1, 3)
    return np.stack([np.linalg.norm(X[:, c] - X[:, p], axis=1) for c, p in bones], axis=1)


def random_rotations(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q


def rigid_row(rng, J, bones, body, root_range=3.0, roots=None, dirs=None):
    """One rigid skeleton [J, 3] in float64: the roots uniform within root_range metres (or roots[j]), bone b a random rotation of its
    body vector (or |body_b| dirs[b], a given unit direction)."""
    pos = np.zeros((J, 3))
    children = [c for c, _ in bones]
    for j in range(J):
        if j not in children:
            pos[j] = rng.uniform(-root_range, root_range, 3) if roots is None or j not in roots else roots[j]
    for k, ((c, p), b) in enumerate(zip(bones, body)):
        b = np.asarray(b, dtype=np.float64)
        q = random_rotations(rng, 1)[0]
        pos[c] = pos[p] + (q @ b if dirs is None or k not in dirs else np.linalg.norm(b) * np.asarray(dirs[k], dtype=np.float64))
    return pos


def rigid_rows(rng, n, J, bones, body, root_range=3.0):
    """n float32 rows [n, 3 J] of rigid_row skeletons (float64 inside, one float32 rounding)."""
    return np.stack([rigid_row(rng, J, bones, body, root_range).ravel() for _ in range(n)]).astype(np.float32)
