"""float64 numpy restatement of dense inference's causal filter (the recipes in include/mmego_hip.h: mmego_one_euro,
mmego_one_euro_bones), written frame by frame with plain loops and plain multiplies and adds (the kernel spells them as fused
multiply-adds: the two differ by roundings of 2^-53, far inside the tests' float bound).  A helper for tests/test_one_euro_ref_cpu.py,
test_one_euro_gpu.py and test_dense_online_gpu.py."""
import numpy as np

TINY = 1e-9


def alpha(fc):
    """The newest sample's weight of an exponential filter of cutoff fc cycles per frame: w / (w + 1), w = 2 pi fc."""
    w = 2.0 * np.pi * np.asarray(fc, dtype=np.float64)
    return w / (w + 1.0)


def runs_of(seg):
    """-> (run_off [R + 1] int64, run_on [R] int32): the maximal stretches of equal seg, which partition [0, F); on where seg >= 0."""
    seg = np.asarray(seg)
    off = [0] + [f for f in range(1, len(seg)) if seg[f] != seg[f - 1]] + [len(seg)]
    return np.asarray(off, dtype=np.int64), np.asarray([1 if seg[a] >= 0 else 0 for a in off[:-1]], dtype=np.int32)


def filter_vectors(x, fc, beta, dc):
    """The recursion on one run of 3-vectors x [n, ..., 3] (float64), every leading axis a joint of its own.  -> xhat [n, ..., 3]."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    out[0] = x[0]
    xhat, dhat, ad = x[0].copy(), np.zeros_like(x[0]), alpha(dc)
    for i in range(1, len(x)):
        d = x[i] - xhat
        dhat = dhat + ad * (d - dhat)
        s = np.sqrt((dhat * dhat).sum(axis=-1, keepdims=True))
        xhat = xhat + alpha(fc + beta * s) * d
        out[i] = xhat
    return out


def one_euro(src, runs, fc, beta, dc):
    """-> (dst [F, 3 J] float64, moved [F] float64) of mmego_one_euro."""
    src = np.asarray(src, dtype=np.float64)
    F, C = src.shape
    dst, moved = src.copy(), np.zeros(F)
    off, on = runs
    for r in range(len(on)):
        a, e = int(off[r]), int(off[r + 1])
        if not on[r]:
            continue
        y = filter_vectors(src[a:e].reshape(e - a, C // 3, 3), fc, beta, dc)
        dst[a:e] = y.reshape(e - a, C)
        moved[a:e] = np.sqrt(((y - src[a:e].reshape(e - a, C // 3, 3)) ** 2).sum(axis=(1, 2)) / (C // 3))
        moved[a] = 0.0
    return dst, moved


def one_euro_bones(src, runs, fc, beta, dc, bones, L):
    """-> (dst [F, 3 J] float64, moved [F], fallback [F] int) of mmego_one_euro_bones; bones [NB, 2] of (child, parent), parents first."""
    src = np.asarray(src, dtype=np.float64)
    F, C = src.shape
    J = C // 3
    x = src.reshape(F, J, 3)
    dst, moved, fell = x.copy(), np.zeros(F), np.zeros(F, dtype=np.int64)
    off, on = runs
    children = [int(c) for c, _ in bones]
    roots = [j for j in range(J) if j not in children]
    for r in range(len(on)):
        a, e = int(off[r]), int(off[r + 1])
        if not on[r] or e - a < 2:
            continue
        pos = np.zeros((e - a, J, 3))
        pos[:, roots] = filter_vectors(x[a:e][:, roots], fc, beta, dc)
        v = np.stack([x[a:e, c] - x[a:e, p] for c, p in bones], axis=1) if len(bones) else np.zeros((e - a, 0, 3))
        vhat = filter_vectors(v, fc, beta, dc) if len(bones) else v
        for i in range(1, e - a):
            for b, (c, p) in enumerate(bones):
                n = np.linalg.norm(vhat[i, b])
                if n > TINY * L[b] and n > 0.0:
                    u = vhat[i, b] / n
                else:
                    fell[a + i] += 1
                    m = np.linalg.norm(v[i, b])
                    u = v[i, b] / m if m > 0.0 else np.zeros(3)
                pos[i, c] = pos[i, p] + float(L[b]) * u
        dst[a + 1:e] = pos[1:]
        moved[a + 1:e] = np.sqrt(((pos[1:] - x[a + 1:e]) ** 2).sum(axis=(1, 2)) / J)
    return dst.reshape(F, C), moved, fell
