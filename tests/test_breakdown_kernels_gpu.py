"""GPU: mmego_colsum_groups and mmego_hist_groups (csrc/breakdown.hip) against the numpy restatement of tests/breakdown_ref.py.

Grouped sums: |out - ref| <= 2^-23 * (the group's sum of |x|) per column, ref in float64 -- the kernel accumulates in double (its error
is negligible at these sizes) and rounds once to fp32, at most 2^-24 |ref|; the bound is twice that over a quantity that cannot cancel.
Counts and histograms: integer equality.  Two launches: the same bits."""
import numpy as np
import pytest
import torch

import breakdown_ref as ref

pytestmark = pytest.mark.gpu

SENT = -12345.0
GARBAGE = -77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _d(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ids(rng, rows, G, kind):
    """Group ids: sorted; shuffled; with -1 and ids >= G mixed in (group G - 2, where there is one, stays empty in all three); one group
    owning every row; every row outside."""
    if kind == "sorted":
        g = np.sort(rng.integers(0, G, rows))
    elif kind == "shuffled":
        g = rng.integers(0, G, rows)
    elif kind == "mixed":
        g = rng.integers(-1, G + 2, rows)
    elif kind == "one":
        g = np.full(rows, G - 1)
    else:
        g = np.where(np.arange(rows) % 2 == 0, -1, G)
    if G >= 3 and kind in ("sorted", "shuffled", "mixed"):
        g = np.where(g == G - 2, G - 1, g)                 # an empty group
    return g.astype(np.int32)


def _table(rng, rows, C, pad, group, G):
    """[rows, C + pad] values in (-100, 100); the rows outside every group hold NaN and +-Inf."""
    X = rng.uniform(-100.0, 100.0, (rows, C + pad)).astype(np.float32)
    out = (group < 0) | (group >= G)
    X[out] = np.where(np.arange(C + pad) % 3 == 0, np.nan, np.where(np.arange(C + pad) % 3 == 1, np.inf, -np.inf)).astype(np.float32)
    return X


@pytest.mark.parametrize("kind", ["sorted", "shuffled", "mixed", "one", "outside"])
@pytest.mark.parametrize("G", [1, 3, 13, 200])
def test_grouped_sums_against_float64(dev, G, kind):
    from mmego_amd import ops
    rng = np.random.default_rng(1000 * G + len(kind))
    worst = 0.0
    for rows in (1, 63, 1025, 5000):
        for C in (1, 43, 64):
            group = _ids(rng, rows, G, kind)
            X = _table(rng, rows, C, 3, group, G)
            Xd = _d(dev, X)
            out = torch.full((G + 1, C + 2), SENT, dtype=torch.float32, device=dev)        # (ldx > C, ldo > C; one more row behind: it stays)
            count = torch.full((G + 1,), SENT, dtype=torch.float32, device=dev)
            ops.colsum_groups(Xd[:, :C], _d(dev, group), G, out[:G], count[:G])
            again = torch.full((G, C + 2), SENT, dtype=torch.float32, device=dev)
            ops.colsum_groups(Xd[:, :C], _d(dev, group), G, again, None)                    # (count is optional)
            assert torch.equal(out[:G], again), "two launches give the same bits"
            o, n = out.cpu().numpy(), count.cpu().numpy()
            sums, mag, cnt = ref.colsum_groups(X[:, :C], group, G)
            assert np.isfinite(o).all(), "a NaN or Inf of a row outside every group reached a sum"
            assert (o[:G, C:] == SENT).all() and (o[G] == SENT).all() and n[G] == SENT, "outputs beyond column C and row G keep their bytes"
            assert np.array_equal(n[:G], cnt.astype(np.float32))
            assert (o[:G, :C][cnt == 0] == 0.0).all(), "a group without rows gets zeros"
            err, bound = np.abs(o[:G, :C].astype(np.float64) - sums), 2.0 ** -23 * mag
            assert (err <= bound).all(), (rows, C, G, kind, float((err - bound).max()))
            worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
    print("colsum_groups G %d %s: worst error / bound %.3f" % (G, kind, worst))


def _values(rng, rows, C, inv_width, nbins):
    """Non-negative values across and beyond the range, then exact bin edges k / inv_width (the product is exact for a power-of-two
    inv_width), zeros, negatives, NaN, +Inf and values far beyond the range sprinkled in."""
    X = (rng.uniform(0.0, 1.25 * nbins, (rows, C)) / inv_width).astype(np.float32)
    flat = X.reshape(-1)
    n = flat.size
    pick = lambda frac: rng.choice(n, max(1, int(frac * n)), replace=False)
    idx = pick(0.2)
    flat[idx] = (rng.integers(0, nbins + 2, len(idx)) / np.float64(inv_width)).astype(np.float32)
    for value, frac in ((0.0, 0.03), (-0.0, 0.01), (-1.5, 0.03), (-1e-30, 0.01), (np.nan, 0.03), (np.inf, 0.02), (3e38, 0.01)):
        flat[pick(frac)] = value
    return X


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("nbins", [1, 2, 300, 4096])
def test_histograms_are_exact(dev, nbins, pool, grouped):
    from mmego_amd import ops
    rng = np.random.default_rng(7 * nbins + 2 * pool + grouped)
    for rows in (1, 64, 5000):
        for C in (1, 21):
            for inv_width in (16.0, 2000.0):               # a power of two (edge values have exact products) and --breakdown's own
                G = 5 if grouped else 1
                group = rng.integers(-1, G + 1, rows).astype(np.int32) if grouped else None
                X = _values(rng, rows, C, inv_width, nbins)
                Xd = _d(dev, np.concatenate([X, np.full((rows, 2), np.nan, np.float32)], axis=1))[:, :C]        # (ldx > C)
                shape = (G, nbins) if pool else (G, C, nbins)
                hist = torch.full(shape, GARBAGE, dtype=torch.int32, device=dev)           # garbage: every word is overwritten
                lost = torch.full(shape[:-1], GARBAGE, dtype=torch.int32, device=dev)
                ops.hist_groups(Xd, None if group is None else _d(dev, group), G, inv_width, nbins, hist, lost, pool=pool)
                h2, l2 = torch.full_like(hist, 5), torch.full_like(lost, 5)
                ops.hist_groups(Xd, None if group is None else _d(dev, group), G, inv_width, nbins, h2, l2, pool=pool)
                assert torch.equal(hist, h2) and torch.equal(lost, l2)
                want, want_lost = ref.hist_groups(X, group, G, inv_width, nbins, pool)
                assert np.array_equal(hist.cpu().numpy(), want), (rows, C, nbins, pool, grouped, inv_width)
                assert np.array_equal(lost.cpu().numpy(), want_lost), (rows, C, nbins, pool, grouped, inv_width)
                inside = rows if group is None else int(((group >= 0) & (group < G)).sum())
                assert int(want.sum() + want_lost.sum()) == inside * C


def test_values_on_bin_edges_land_in_the_upper_bin(dev):
    from mmego_amd import ops
    nbins, inv_width = 8, 4.0
    x = np.asarray([0.0, 0.25, 0.4999999, 0.5, 1.5, 1.75, 1.7499999, 2.0, 100.0, np.inf, -0.0, -0.25, np.nan], dtype=np.float32)
    hist = torch.full((1, nbins), GARBAGE, dtype=torch.int32, device=dev)
    lost = torch.full((1,), GARBAGE, dtype=torch.int32, device=dev)
    ops.hist_groups(_d(dev, np.stack([x, -x], axis=1))[:, :1], None, 1, inv_width, nbins, hist, lost)      # (one column of two: ldx = 2)
    assert hist.cpu().numpy().tolist() == [[2, 2, 1, 0, 0, 0, 2, 4]] and lost.cpu().numpy().tolist() == [2]
    assert ref.bins(x, inv_width, nbins).tolist() == [0, 1, 1, 2, 6, 7, 6, 7, 7, 7, 0, -1, -1]


def test_entry_points_refuse_bad_arguments(dev):
    """Every refusal: a non-zero return (hip.call raises "bad argument"), nothing launched, the sentinels stay."""
    from mmego_amd import hip
    rows, C, G, nbins = 40, 21, 3, 16
    X = torch.ones((rows, 24), dtype=torch.float32, device=dev)
    group = torch.zeros(rows, dtype=torch.int32, device=dev)
    out = torch.full((G, 24), SENT, dtype=torch.float32, device=dev)
    count = torch.full((G,), SENT, dtype=torch.float32, device=dev)
    good = dict(X=X, ldx=24, rows=rows, C=C, group=group, G=G, out=out, ldo=24, count=count)
    bad = [dict(X=None), dict(group=None), dict(out=None), dict(C=0), dict(C=65, ldx=65, ldo=65), dict(G=0), dict(G=65536), dict(ldx=C - 1),
           dict(ldo=C - 1), dict(rows=0), dict(rows=1 << 24), dict(rows=-1)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("colsum_groups", *[a[k] for k in good])
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((count == SENT).all())
    hip.call("colsum_groups", *[dict(good, count=None)[k] for k in good])                   # (count is optional)
    assert bool((out[0, :C] == rows).all()) and not out[1:, :C].any() and bool((out[:, C:] == SENT).all()) and bool((count == SENT).all())
    hist = torch.full((G, nbins), GARBAGE, dtype=torch.int32, device=dev)
    lost = torch.full((G,), GARBAGE, dtype=torch.int32, device=dev)
    good = dict(X=X, ldx=24, rows=rows, C=C, group=group, G=G, inv_width=2.0, nbins=nbins, pool=1, hist=hist, dropped=lost)
    bad = [dict(X=None), dict(hist=None), dict(dropped=None), dict(group=None), dict(C=0), dict(C=65, ldx=65), dict(G=0), dict(G=65536),
           dict(nbins=0), dict(nbins=4097), dict(ldx=C - 1), dict(rows=0), dict(rows=1 << 24), dict(pool=2), dict(inv_width=0.0),
           dict(inv_width=-1.0), dict(inv_width=float("inf")), dict(inv_width=float("nan"))]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("hist_groups", *[a[k] for k in good])
    torch.cuda.synchronize()
    assert bool((hist == GARBAGE).all()) and bool((lost == GARBAGE).all())
    hip.call("hist_groups", *[dict(good, group=None, G=1)[k] for k in good])                # (a NULL group is one group of all rows)
    assert int(hist[0, 2]) == rows * C and int(hist[0].sum()) == rows * C and int(lost[0]) == 0 and bool((hist[1:] == GARBAGE).all())


def test_wrappers_raise_before_launching(dev):
    from mmego_amd import ops
    X = torch.ones((40, 21), dtype=torch.float32, device=dev)
    group = torch.zeros(40, dtype=torch.int32, device=dev)
    out = torch.full((3, 21), SENT, dtype=torch.float32, device=dev)
    count = torch.full((3,), SENT, dtype=torch.float32, device=dev)
    hist = torch.full((3, 16), GARBAGE, dtype=torch.int32, device=dev)
    lost = torch.full((3,), GARBAGE, dtype=torch.int32, device=dev)
    wide = torch.ones((40, 65), dtype=torch.float32, device=dev)
    for kind, call in (
            (TypeError, lambda: ops.colsum_groups(X.double(), group, 3, out)),
            (TypeError, lambda: ops.colsum_groups(X.cpu(), group, 3, out)),
            (TypeError, lambda: ops.colsum_groups(X, group.long(), 3, out)),
            (TypeError, lambda: ops.colsum_groups(X, group.cpu(), 3, out)),
            (TypeError, lambda: ops.colsum_groups(X, None, 3, out)),
            (TypeError, lambda: ops.colsum_groups(X, group, 3.0, out)),
            (TypeError, lambda: ops.colsum_groups(X, group, 3, out, count.double())),
            (ValueError, lambda: ops.colsum_groups(X, group[:39], 3, out)),
            (ValueError, lambda: ops.colsum_groups(X, group, 0, out)),
            (ValueError, lambda: ops.colsum_groups(X, group, 65536, out)),
            (ValueError, lambda: ops.colsum_groups(X, group, 2, out)),
            (ValueError, lambda: ops.colsum_groups(X, group, 3, out[:, :20])),
            (ValueError, lambda: ops.colsum_groups(X, group, 3, out, count[:2])),
            (ValueError, lambda: ops.colsum_groups(wide, group, 3, out)),
            (ValueError, lambda: ops.colsum_groups(X.t(), group, 3, out)),
            (ValueError, lambda: ops.colsum_groups(X[:0], group[:0], 3, out)),
            (TypeError, lambda: ops.hist_groups(X, group, 3, 2.0, 16, hist.float(), lost)),
            (TypeError, lambda: ops.hist_groups(X, group, 3, 2.0, 16, hist, lost.long())),
            (TypeError, lambda: ops.hist_groups(X, group, 3, 2.0, 16.0, hist, lost)),
            (TypeError, lambda: ops.hist_groups(X, group, 3, "2", 16, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, None, 3, 2.0, 16, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, 2.0, 0, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, 2.0, 4097, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, 0.0, 16, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, -2.0, 16, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, float("nan"), 16, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, float("inf"), 16, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, 1.0 / 3.0, 16, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, 2.0, 16, hist, lost, pool=False)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, 2.0, 8, hist, lost)),
            (ValueError, lambda: ops.hist_groups(X, group, 3, 2.0, 16, hist, lost[:2]))):
        with pytest.raises(kind):
            call()
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((count == SENT).all()) and bool((hist == GARBAGE).all()) and bool((lost == GARBAGE).all())
