"""float64 numpy restatement of dense inference's host plan and of its two kernels (the recipes in mmego_amd/data.py DensePlan and in
include/mmego_hip.h: mmego_blend_windows, mmego_colsum_phase), written frame by frame with plain loops -- another route than the
vectorised plan and the lane-per-column kernels.  A helper for tests/test_dense_plan_cpu.py, test_blend_gpu.py, test_dense_infer_gpu.py."""
import numpy as np


def window_starts(lengths, T, S):
    """Per recording occupying [a, b): none if b - a < T, else {b - T - k S >= a} united with {a}, ascending; recording by recording."""
    starts, a = [], 0
    for n in lengths:
        b = a + int(n)
        if b - a >= T:
            s, k = {a}, 0
            while b - T - k * S >= a:
                s.add(b - T - k * S)
                k += 1
            starts.extend(sorted(s))
        a = b
    return np.asarray(starts, dtype=np.int64)


def cover(starts, T, F, blend):
    """-> (cov_off [F + 1], cov_row [nnz], cov_w [nnz]): for every frame the rows w T + p of the windows that hold it, ascending w."""
    lists = [[] for _ in range(F)]
    for w, s in enumerate(starts):
        for p in range(T):
            lists[int(s) + p].append((w * T + p, 1.0 if blend == "mean" else float(min(p + 1, T - p))))
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    row = np.asarray([r for l in lists for r, _ in l], dtype=np.int32)
    wt = np.asarray([v for l in lists for _, v in l], dtype=np.float32)
    return off, row, wt


def blend(src, off, row, w, spread=True):
    """-> (dst [F, C] float64, spread [F] float64 or None) of mmego_blend_windows."""
    src = np.asarray(src, dtype=np.float64)
    F, C = len(off) - 1, src.shape[1]
    dst, spr = np.zeros((F, C)), np.zeros(F)
    for f in range(F):
        k = slice(int(off[f]), int(off[f + 1]))
        wk = np.asarray(w[k], dtype=np.float64)
        if wk.size == 0 or wk.sum() == 0.0:
            continue
        x = src[np.asarray(row[k], dtype=np.int64)]
        m = (wk[:, None] * x).sum(axis=0) / wk.sum()
        dst[f] = m
        if spread:
            d2 = ((x - m) ** 2).reshape(len(wk), C // 3, 3).sum(axis=2)          # |x_kj - m_j|^2
            spr[f] = np.sqrt((wk[:, None] * d2).sum() / ((C // 3) * wk.sum()))
    return dst, (spr if spread else None)


def colsum_phase(X, period):
    """-> [period, C] float64: out[p] = sum of the rows r = p (mod period)."""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([X[p::period].sum(axis=0) for p in range(period)])


def within(out, want):
    """The worst |out - want| in units of the bound 2^-23 |want| + 1e-7 of the double-inside, float-store kernels (<= 1: inside)."""
    out, want = np.asarray(out, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if out.size == 0:
        return 0.0
    return float((np.abs(out - want) / (2.0 ** -23 * np.abs(want) + 1e-7)).max())


UPPER_MAP = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 20)
LOWER_MAP = (12, 13, 14, 15, 16, 17, 18, 19)


def assemble(up, lo):
    """[n, 15, 3], [n, 8, 3] -> the 21-joint skeleton (lower overwrites the shared hips)."""
    up, lo = np.asarray(up, dtype=np.float64).reshape(-1, 15, 3), np.asarray(lo, dtype=np.float64).reshape(-1, 8, 3)
    p = np.zeros((len(up), 21, 3))
    p[:, list(UPPER_MAP)] = up
    p[:, list(LOWER_MAP)] = lo
    return p


def errors_cm(up, lo, target):
    """The reference's joint errors in float64 from unassembled rows: (all, upper, lower) means in cm and the per-row 21-joint mean
    [n] in cm.  upper: the 15 upper joints of `up` itself against target[UPPER_MAP] (the hips as the Upper net placed them)."""
    t = np.asarray(target, dtype=np.float64).reshape(-1, 21, 3)
    upj, loj = np.asarray(up, dtype=np.float64).reshape(-1, 15, 3), np.asarray(lo, dtype=np.float64).reshape(-1, 8, 3)
    e = np.linalg.norm(assemble(up, lo) - t, axis=2)
    eu = np.linalg.norm(upj - t[:, list(UPPER_MAP)], axis=2)
    el = np.linalg.norm(loj - t[:, list(LOWER_MAP)], axis=2)
    return float(e.mean()) * 100, float(eu.mean()) * 100, float(el.mean()) * 100, e.mean(axis=1) * 100
