"""Numpy restatement of mmego_colsum_groups / mmego_hist_groups (include/mmego_hip.h) and of the host helpers of the error breakdown
(mmego_amd/evaluation.py), for the tests: grouped sums in float64, the histogram by the kernel's own fp32 recipe with its comparisons in
the same order, quantiles as order statistics."""
import numpy as np


def colsum_groups(X, group, G):
    """-> (sums [G, C] float64, sum of |x| [G, C] float64, counts [G] int64) of the rows whose id lies in [0, G); others are never read."""
    X, group = np.asarray(X), np.asarray(group)
    C = X.shape[1]
    sums, mag, count = np.zeros((G, C)), np.zeros((G, C)), np.zeros(G, dtype=np.int64)
    for g in range(G):
        rows = X[group == g].astype(np.float64)
        sums[g], mag[g], count[g] = rows.sum(axis=0), np.abs(rows).sum(axis=0), len(rows)
    return sums, mag, count


def bins(x, inv_width, nbins):
    """The bin of every value of x (fp32): -1 where it is NaN or < 0; nbins - 1 where the fp32 product x * inv_width >= nbins - 1 (+Inf
    too), decided before any conversion to an integer; else int(x * inv_width)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (x * np.float32(inv_width)).astype(np.float32)
    out = np.full(x.shape, -1, dtype=np.int64)
    counted = ~(np.isnan(x) | (x < np.float32(0)))
    over = counted & (t >= np.float32(nbins - 1))
    out[over] = nbins - 1
    rest = counted & ~over
    out[rest] = t[rest].astype(np.int64)                                 # (truncation; the values are >= 0 and < nbins - 1)
    return out


def hist_groups(X, group, G, inv_width, nbins, pool):
    """-> (hist, dropped): [G, nbins] and [G] pooled over the columns, [G, C, nbins] and [G, C] per column; group None: one group."""
    X = np.asarray(X, dtype=np.float32)
    rows, C = X.shape
    group = np.zeros(rows, dtype=np.int64) if group is None else np.asarray(group)
    b = bins(X, inv_width, nbins)
    hist, dropped = np.zeros((G, C, nbins), dtype=np.int64), np.zeros((G, C), dtype=np.int64)
    for g in range(G):
        for c in range(C):
            v = b[group == g, c]
            dropped[g, c] = np.count_nonzero(v < 0)
            hist[g, c] = np.bincount(v[v >= 0], minlength=nbins)
    return (hist.sum(axis=1), dropped.sum(axis=1)) if pool else (hist, dropped)


def order_statistic(x, q):
    """x_(ceil(q n)) of the values x, in float64 (1-based: the smallest value with at least q n values <= it)."""
    x = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    return float(x[max(int(np.ceil(q * len(x))), 1) - 1])


def pck_auc(hist, bin_width, upto=15.0):
    """The mean over the bin edges k * bin_width <= upto (to a relative 1e-9), 1 <= k <= nbins - 1, of cum[k - 1] / n; None without one."""
    hist = np.asarray(hist, dtype=np.int64)
    n, K = int(hist.sum()), int(min(np.floor(upto / bin_width * (1.0 + 1e-9)), len(hist) - 1))
    if n == 0 or K < 1:
        return None
    cum = np.cumsum(hist)
    return float(sum(float(cum[k - 1]) for k in range(1, K + 1)) / (float(n) * K))


BONES_ALL = ((20, 3), (3, 2), (2, 1), (2, 4), (2, 8), (4, 5), (5, 6), (6, 7), (8, 9), (9, 10), (10, 11), (1, 0), (0, 12), (0, 16),
             (12, 13), (13, 14), (14, 15), (16, 17), (17, 18), (18, 19))                      # (parent, child) in the 21-joint numbering


def bone_angles_deg(pred, target):
    """[n, 21, 3] x 2 -> [n, 20] float64: the angle in degrees between every predicted bone and the recorded one (Demo_test.py:64-69)."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    root, leaf = [b[0] for b in BONES_ALL], [b[1] for b in BONES_ALL]
    u, v = p[:, leaf] - p[:, root], t[:, leaf] - t[:, root]
    cs = (u * v).sum(-1) / (np.maximum(np.linalg.norm(u, axis=-1), 1e-8) * np.maximum(np.linalg.norm(v, axis=-1), 1e-8))
    return np.abs(np.degrees(np.arccos(np.clip(cs, -1.0, 1.0))))
