"""GPU: the two kernels of dense inference (csrc/blend.hip) -- mmego_blend_windows, every frame's row blended from the window rows
that cover it, and mmego_colsum_phase, a per-row table folded by position in the window -- against the float64 restatement of
tests/dense_ref.py.

Bound on every element: |out - ref| <= 2^-23 |ref| + 1e-7, the bound tests/test_pose_metrics_gpu.py holds the double-inside,
float-store kernels to (the float store, and a floor far above what the double sums leave)."""
import numpy as np
import pytest
import torch

import dense_ref as ref

pytestmark = pytest.mark.gpu

SENT = -12345.0
NROWS = 400


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _d(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cover(rng, F, weights):
    """Covers of 0 .. 21 rows per frame: frame 0 empty, frame 1 (if any) covered once, and -- from three frames on -- one row listed by
    two frames.  weights: ones, the triangle of a 20-frame window by list position, or random in (0.5, 2)."""
    counts = rng.integers(0, 22, F)
    counts[0] = 0
    if F > 1:
        counts[1] = 1
    if F > 2:
        counts[2] = max(counts[2], 2)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    row = rng.integers(0, NROWS, int(off[-1])).astype(np.int32)
    if F > 2:
        row[off[2]] = row[off[1]]                      # the singly covered frame's row is in the next frame's list as well
    p = np.concatenate([np.arange(c) % 20 for c in counts]) if off[-1] else np.zeros(0, np.int64)
    w = {"ones": np.ones(len(row)), "triangle": np.minimum(p + 1, 20 - p), "random": rng.uniform(0.5, 2.0, len(row))}[weights]
    return off, row, w.astype(np.float32)


def _blend(dev, src, cover, pad, spread=True):
    from mmego_amd import ops
    F, C = len(cover[0]) - 1, src.shape[1]
    dst = torch.full((F + 1, C + pad), SENT, dtype=torch.float32, device=dev)        # (one more row behind the last: it stays)
    spr = torch.full((F + 1,), SENT, dtype=torch.float32, device=dev)
    ops.blend_windows(_d(dev, src), cover, dst[:F], spr[:F] if spread else None)
    return dst, spr


@pytest.mark.parametrize("weights", ["ones", "triangle", "random"])
@pytest.mark.parametrize("C", [24, 45, 63])
@pytest.mark.parametrize("F", [1, 3, 64, 65, 257])
def test_blend_against_the_restatement(dev, F, C, weights):
    rng = np.random.default_rng(1000 * F + 10 * C + len(weights))
    src = rng.normal(0.0, 0.7, (NROWS, C)).astype(np.float32)
    cover = _cover(rng, F, weights)
    off, row, w = cover
    want, want_spr = ref.blend(src, off, row, w)
    for pad in (0, 3):
        dst, spr = _blend(dev, src, cover, pad)
        out, s = dst.cpu().numpy(), spr.cpu().numpy()
        assert np.all(out[:F, C:] == SENT) and np.all(out[F] == SENT) and s[F] == SENT, "written outside the F rows of C columns"
        worst, worst_s = ref.within(out[:F, :C], want), ref.within(s[:F], want_spr)
        print("F %d C %d %s ldd C+%d: worst error / bound %.3f (dst) %.3f (spread)" % (F, C, weights, pad, worst, worst_s))
        assert worst <= 1.0 and worst_s <= 1.0, (pad, worst, worst_s)
        assert not np.isnan(out).any() and not np.isnan(s).any()
        assert not out[0, :C].any() and s[0] == 0.0, "an empty list gives a zero row and spread 0"
        # frames covered once: their row, bit for bit
        once = np.flatnonzero(np.diff(off) == 1)
        assert len(once) >= min(F - 1, 1)
        assert torch.equal(dst[:F, :C][_d(dev, once)], _d(dev, src)[_d(dev, row[off[once]].astype(np.int64))])
        assert np.all(s[once] == 0.0)
        # two launches, the same bits
        dst2, spr2 = _blend(dev, src, cover, pad)
        assert torch.equal(dst, dst2) and torch.equal(spr, spr2)
    # without spread: the same dst, the spread buffer untouched
    dst3, spr3 = _blend(dev, src, cover, 0, spread=False)
    assert torch.equal(dst3, _blend(dev, src, cover, 0)[0]) and bool((spr3 == SENT).all())


def test_blend_takes_the_plan_object_and_64_columns(dev):
    from mmego_amd import ops
    from mmego_amd.data import DensePlan
    plan = DensePlan([5, 20, 23, 41], 20, 7, "triangle")
    rng = np.random.default_rng(3)
    src = rng.normal(size=(plan.W * 20, 64)).astype(np.float32)
    dst = torch.full((plan.F, 64), SENT, dtype=torch.float32, device=dev)
    ops.blend_windows(_d(dev, src), plan, dst)
    want, _ = ref.blend(src, plan.cov_off, plan.cov_row, plan.cov_w, spread=False)
    assert ref.within(dst.cpu().numpy(), want) <= 1.0 and not dst[:5].any()
    assert "_cover_dev" in plan.__dict__                                           # (the plan keeps its device copies)
    with pytest.raises(IndexError):                                                # a source shorter than the plan's rows: host check
        ops.blend_windows(_d(dev, src[:-1]), plan, dst)
    with pytest.raises(ValueError):
        ops.blend_windows(_d(dev, src), plan, dst, torch.zeros(plan.F, device=dev))      # spread of rows that are no 3-vectors


@pytest.mark.parametrize("C", [1, 43, 45])
@pytest.mark.parametrize("n", [1, 7, 1000])
@pytest.mark.parametrize("period", [1, 8, 20])
def test_colsum_phase_against_the_restatement(dev, period, n, C):
    from mmego_amd import ops
    rng = np.random.default_rng(100 * period + 10 * n + C)
    for pad in (0, 5):
        X = rng.normal(0.0, 50.0, (n * period, C + pad)).astype(np.float32)
        Xd = _d(dev, X)
        out = torch.full((period + 1, C + 2), SENT, dtype=torch.float32, device=dev)
        ops.colsum_phase(Xd[:, :C], period, out[:period, :C])
        got = out.cpu().numpy()
        assert np.all(got[:period, C:] == SENT) and np.all(got[period] == SENT)
        worst = ref.within(got[:period, :C], ref.colsum_phase(X[:, :C], period))
        print("period %d rows/phase %d C %d ldx C+%d: worst error / bound %.3f" % (period, n, C, pad, worst))
        assert worst <= 1.0, (pad, worst)
        out2 = torch.full_like(out, SENT)
        ops.colsum_phase(Xd[:, :C], period, out2[:period, :C])
        assert torch.equal(out, out2)


def test_refusals_leave_the_outputs_alone(dev):
    """Every refusal of the two entry points: a non-zero return (hip.call raises), nothing launched, the sentinels stay."""
    from mmego_amd import hip
    F, C = 5, 45
    src = torch.zeros((NROWS, C), dtype=torch.float32, device=dev)
    off = _d(dev, np.arange(F + 1, dtype=np.int64))
    row, w = _d(dev, np.arange(F, dtype=np.int32)), torch.ones(F, dtype=torch.float32, device=dev)
    dst = torch.full((F, 64), SENT, dtype=torch.float32, device=dev)
    spr = torch.full((F,), SENT, dtype=torch.float32, device=dev)
    good = dict(src=src, nrows=NROWS, C=C, cov_off=off, cov_row=row, cov_w=w, F=F, dst=dst, ldd=64, spread=spr)
    bad = [dict(src=None), dict(cov_off=None), dict(cov_row=None), dict(cov_w=None), dict(dst=None), dict(F=0), dict(F=-1), dict(C=0),
           dict(C=65, ldd=65), dict(ldd=C - 1), dict(C=44, spread=spr), dict(C=1, spread=spr)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("blend_windows", *[a[k] for k in good])
    hip.call("blend_windows", *[dict(good, C=44, spread=None)[k] for k in good])         # (44 columns are fine without spread)
    torch.cuda.synchronize()
    assert bool((dst[:, 44:] == SENT).all()) and bool((spr == SENT).all()) and not dst[:, :44].any()
    dst.fill_(SENT)
    X = torch.ones((40, 45), dtype=torch.float32, device=dev)
    out = torch.full((20, 45), SENT, dtype=torch.float32, device=dev)
    good = dict(X=X, ldx=45, rows=40, C=45, period=20, out=out, ldo=45)
    bad = [dict(X=None), dict(out=None), dict(rows=0), dict(rows=41), dict(period=0), dict(period=65, rows=65), dict(C=0), dict(C=65),
           dict(ldx=44), dict(ldo=44)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("colsum_phase", *[a[k] for k in good])
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((dst == SENT).all())
    hip.call("colsum_phase", *good.values())
    assert bool((out == 2.0).all())
