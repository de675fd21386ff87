"""CPU: the float64 restatement of dense inference's temporal filter (tests/smooth_ref.py) checked on its own, by properties that do not
depend on how the coefficients are computed: they sum to 1, a polynomial of degree <= D comes back unchanged (at segment edges and array
ends too), D = 0 under the box taper is the plain moving average, and in the interior the filter is scipy's Savitzky-Golay filter."""
import numpy as np
import pytest

import smooth_ref as sref

HS = (1, 2, 3, 5, 8, 16, 31)


def _truncations(H):
    """Every one-sided truncation: a left reach of 0 .. H with a right reach in {0, 1, H // 2, H}."""
    return [list(range(-left, right + 1)) for left in range(H + 1) for right in sorted({0, 1, H // 2, H})]


@pytest.mark.parametrize("taper", ["box", "gauss"])
@pytest.mark.parametrize("H", HS)
def test_coefficients_sum_to_one_and_stay_small(H, taper):
    w = sref.weights(H, taper)
    worst = 0.0
    for D in (0, 1, 2):
        for taps in _truncations(H):
            c = sref.coefficients(w, taps, D)
            assert c.shape == (len(taps),) and abs(c.sum() - 1.0) <= 1e-12, (D, taps)
            worst = max(worst, float(np.abs(c).sum()))
            if len(taps) == 1:
                assert c[0] == pytest.approx(1.0, abs=1e-15)
    print("H %d %s: largest sum |c_k| %.4f" % (H, taper, worst))
    assert worst <= 2.03 + 1e-9         # (a quadratic evaluated at the end of a one-sided window)


@pytest.mark.parametrize("taper", ["box", "gauss"])
@pytest.mark.parametrize("D", [0, 1, 2])
def test_polynomials_of_degree_D_come_back(D, taper):
    rng = np.random.default_rng(D)
    for H in (1, 3, 8, 31):
        F = 90
        seg = np.repeat([0, 1, -1, 4, 2, 3], [40, 17, 3, 2, 1, 27]).astype(np.int32)
        assert len(seg) == F
        t = (np.arange(F) - 45.0) / 30.0
        coef = rng.normal(size=(D + 1, 6))
        x = sum(coef[m] * t[:, None] ** m for m in range(D + 1))
        y, moved = sref.smooth_frames(x, seg, sref.weights(H, taper), D)
        # (fewer than D + 1 valid taps: the fit of degree n - 1 interpolates its n points, the frame's own value comes back too)
        assert np.abs(y - x).max() <= 1e-11 * max(1.0, np.abs(x).max()), (H, D)
        assert np.array_equal(y[seg < 0], x[seg < 0]) and np.array_equal(y[seg == 2], x[seg == 2]) and moved[62] == 0.0


def test_degree_zero_box_is_the_moving_average():
    rng = np.random.default_rng(1)
    F, H = 50, 4
    x = rng.normal(size=(F, 9))
    seg = np.repeat([0, 1], [30, 20]).astype(np.int32)
    y, moved = sref.smooth_frames(x, seg, sref.weights(H, "box"), 0)
    for f in range(F):
        lo, hi = (0, 30) if f < 30 else (30, 50)
        a, b = max(lo, f - H), min(hi, f + H + 1)
        assert np.allclose(y[f], x[a:b].mean(axis=0), rtol=0, atol=1e-14), f
        assert np.isclose(moved[f], np.sqrt(((y[f] - x[f]) ** 2).sum() / 3), rtol=1e-14)


def test_the_interior_is_savitzky_golay():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(2)
    F = 80
    x = rng.normal(size=(F, 5))
    seg = np.zeros(F, np.int32)
    for H in (1, 2, 5, 16):
        for D in (0, 1, 2):
            if D > 2 * H:
                continue
            y, _ = sref.smooth_frames(x, seg, sref.weights(H, "box"), D)
            want = signal.savgol_filter(x, 2 * H + 1, D, axis=0, mode="interp")
            assert np.abs(y - want)[H:F - H].max() <= 1e-12, (H, D)


def test_bones_form_on_a_case_worked_by_hand():
    """A chain 0 -> 1 of length 1 seen along x, then y, then x again under a box moving average (D = 0): the middle frame's bone lies along
    (2, 1) / sqrt 5 at length 1 where the column filter leaves it sqrt 5 / 3 long; the root is the mean.  A bone that reverses between
    two frames cancels and keeps its own frame's direction."""
    bones, L = ((1, 0),), np.array([1.0], np.float32)
    src = np.array([[0, 0, 0, 1, 0, 0], [3, 0, 0, 3, 1, 0], [6, 0, 0, 7, 0, 0]], dtype=np.float64)
    seg = np.zeros(3, np.int32)
    dst, moved, fb = sref.smooth_bones(src, seg, sref.weights(1, "box"), 0, bones, L)
    r5 = np.sqrt(5.0)
    assert np.allclose(dst[1], [3, 0, 0, 3 + 2 / r5, 1 / r5, 0], rtol=0, atol=1e-14) and not fb.any()
    plain, _ = sref.smooth_frames(src, seg, sref.weights(1, "box"), 0)
    assert np.isclose(np.linalg.norm(plain[1, 3:] - plain[1, :3]), r5 / 3)
    assert np.isclose(moved[1], np.sqrt(((dst[1] - src[1]) ** 2).sum() / 2))
    src = np.array([[0, 0, 0, 0.25, 0, 0], [1, 0, 0, 0.75, 0, 0]], dtype=np.float64)
    dst, _, fb = sref.smooth_bones(src, np.zeros(2, np.int32), sref.weights(1, "box"), 0, bones, np.array([0.25], np.float32))
    assert fb.tolist() == [1, 1] and np.allclose(dst, [[0.5, 0, 0, 0.75, 0, 0], [0.5, 0, 0, 0.25, 0, 0]], rtol=0, atol=1e-15)
