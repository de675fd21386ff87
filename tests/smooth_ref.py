"""float64 numpy restatement of dense inference's temporal filter (the recipes in include/mmego_hip.h: mmego_smooth_frames,
mmego_smooth_bones), written frame by frame with plain loops and by ANOTHER ROUTE than the kernel's: the coefficients come from the
pseudo-inverse of the sqrt-weighted Vandermonde matrix on the abscissae k / H (a least-squares solve), not from the moment matrix's
cofactors.  A helper for tests/test_smooth_ref_cpu.py, test_smooth_gpu.py, test_smooth_bones_gpu.py and test_dense_smooth_gpu.py."""
import numpy as np

TINY = 1e-9


def weights(H, taper):
    """box: ones; gauss: exp(-2 k^2 / H^2), rounded to float32 (what dense.smooth_weights returns)."""
    k = np.arange(-H, H + 1, dtype=np.float64)
    return (np.ones(2 * H + 1) if taper == "box" else np.exp(-2.0 * k * k / (H * H))).astype(np.float32)


def valid_taps(seg, f, H):
    """The taps k in [-H, H] of frame f that stay inside the array and inside f's segment (none for seg[f] < 0)."""
    F = len(seg)
    return [k for k in range(-H, H + 1) if 0 <= f + k < F and seg[f] >= 0 and seg[f + k] == seg[f]]


def coefficients(w, taps, D):
    """c_k of the valid taps `taps` (ascending) under the weight table w [2 H + 1]: the row of the weighted least-squares fit of degree
    min(D, len(taps) - 1) that gives the polynomial's value at k = 0."""
    H = len(w) // 2
    k = np.asarray(taps, dtype=np.float64)
    rw = np.sqrt(np.asarray(w, dtype=np.float64)[np.asarray(taps) + H])
    deg = min(D, len(taps) - 1)
    V = np.vander(k / H, deg + 1, increasing=True) * rw[:, None]           # min | rw (V a - x) |, value at 0 = a_0
    return np.linalg.pinv(V)[0] * rw


def smooth_frames(src, seg, w, D):
    """-> (dst [F, C] float64, moved [F] float64) of mmego_smooth_frames (moved: for C % 3 == 0, else zeros)."""
    src = np.asarray(src, dtype=np.float64)
    F, C = src.shape
    H = len(w) // 2
    dst, moved = src.copy(), np.zeros(F)
    for f in range(F):
        taps = valid_taps(seg, f, H)
        if len(taps) <= 1:
            continue
        c = coefficients(w, taps, D)
        y = np.zeros(C)
        for ck, k in zip(c, taps):
            y += ck * src[f + k]
        dst[f] = y
        if C % 3 == 0:
            moved[f] = np.sqrt(((y - src[f]) ** 2).sum() / (C // 3))
    return dst, moved


def smooth_bones(src, seg, w, D, bones, bone_len):
    """-> (dst [F, 3 J] float64, moved [F] float64, fallback [F] int) of mmego_smooth_bones."""
    src = np.asarray(src, dtype=np.float64)
    F, J = src.shape[0], src.shape[1] // 3
    H = len(w) // 2
    dst, moved, fb = src.copy(), np.zeros(F), np.zeros(F, dtype=np.int64)
    children = [c for c, _ in bones]
    for f in range(F):
        taps = valid_taps(seg, f, H)
        if len(taps) <= 1:
            continue
        ck = coefficients(w, taps, D)
        x = [src[f + k].reshape(J, 3) for k in taps]
        own = src[f].reshape(J, 3)
        pos = np.zeros((J, 3))
        for j in range(J):
            if j not in children:
                for c, xk in zip(ck, x):
                    pos[j] += c * xk[j]
        for (c, p), L in zip(bones, bone_len):
            L = float(L)
            s = np.zeros(3)
            for cc, xk in zip(ck, x):
                s += cc * (xk[c] - xk[p])
            n = np.sqrt((s * s).sum())
            if n > TINY * L and n > 0.0:
                u = s / n
            else:
                fb[f] += 1
                d = own[c] - own[p]
                m = np.sqrt((d * d).sum())
                u = d / m if m > 0.0 else np.zeros(3)
            pos[c] = pos[p] + L * u
        dst[f] = pos.ravel()
        moved[f] = np.sqrt(((pos - own) ** 2).sum() / J)
    return dst, moved, fb
