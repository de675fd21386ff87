"""CPU: data.DensePlan's causal cover (lookahead=L) against a brute-force restatement of its definition -- window row r of window
w = r // T, last frame e = starts[w] + T - 1, covers frame f only where e <= f + L -- for recordings of 23, 20, 7 and 41 frames at
T = 20, strides 1 and 3, both blends and every L in 0 .. 19 that the stride allows (stride <= L + 1)."""
import numpy as np
import pytest

from mmego_amd.data import DensePlan

T, LENGTHS = 20, (23, 20, 7, 41)
F = sum(LENGTHS)
ARRAYS = ("starts", "recording", "row_frame", "cov_off", "cov_row", "cov_w", "covered", "rec_off", "frame_rec", "frame_in_recording")
CASES = [(S, blend, L) for S in (1, 3) for blend in ("mean", "triangle") for L in range(T) if S <= L + 1]


def brute(plan, L):
    """The cover of every frame from the definition alone: rows in ascending order, the weights those of the blend."""
    off, rows, wts = [0], [], []
    for f in range(plan.F):
        for r in range(plan.W * T):
            w, p = divmod(r, T)
            if plan.starts[w] + p == f and plan.starts[w] + T - 1 <= f + L:
                rows.append(r)
                wts.append(1.0 if plan.blend == "mean" else float(min(p + 1, T - p)))
        off.append(len(rows))
    return np.asarray(off, np.int64), np.asarray(rows, np.int32), np.asarray(wts, np.float32)


@pytest.mark.parametrize("S,blend,L", CASES)
def test_the_cover_is_the_definition(S, blend, L):
    off_plan, plan = DensePlan(LENGTHS, T, S, blend), DensePlan(LENGTHS, T, S, blend, lookahead=L)
    for name in ("starts", "recording", "row_frame"):
        assert np.array_equal(getattr(plan, name), getattr(off_plan, name)), name
    assert plan.W == off_plan.W and plan.lookahead == L and off_plan.lookahead is None
    off, rows, wts = brute(plan, L)
    assert plan.cov_off.dtype == np.int64 and plan.cov_row.dtype == np.int32 and plan.cov_w.dtype == np.float32
    assert np.array_equal(plan.cov_off, off) and np.array_equal(plan.cov_row, rows) and np.array_equal(plan.cov_w, wts)
    assert np.array_equal(plan.covered, np.diff(off)) and plan.max_cover == np.diff(off).max()
    # the uncovered frames: the first 19 - L of the three long recordings, and the 7-frame recording
    want = np.zeros(F, bool)
    for a, n in zip(plan.rec_off[:-1], LENGTHS):
        want[a:a + (T - 1 - L if n >= T else n)] = True
    assert np.array_equal(plan.covered == 0, want)
    assert plan.warmup == 3 * (T - 1 - L) and off_plan.warmup == 0


@pytest.mark.parametrize("S", [1, 3, 20])
@pytest.mark.parametrize("blend", ["mean", "triangle"])
def test_lookahead_T_minus_1_and_none_are_the_offline_plan(S, blend):
    a = DensePlan(LENGTHS, T, S, blend)
    for other in (DensePlan(LENGTHS, T, S, blend, lookahead=T - 1), DensePlan(LENGTHS, T, S, blend, lookahead=None)):
        for name in ARRAYS:
            x, y = getattr(a, name), getattr(other, name)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
        assert (a.W, a.F, a.max_cover, a.T, a.stride, a.blend) == (other.W, other.F, other.max_cover, other.T, other.stride, other.blend)


def test_stride_1_lookahead_0_is_one_row_at_the_last_position():
    plan = DensePlan(LENGTHS, T, 1, "mean", lookahead=0)
    cov = plan.covered > 0
    assert (plan.covered[cov] == 1).all() and plan.max_cover == 1 and (plan.cov_row % T == T - 1).all()
    assert np.array_equal(plan.row_frame[plan.cov_row], np.flatnonzero(cov))
    assert plan.warmup == 57 and cov.sum() == F - 7 - 57


def test_refusals():
    for S, L in ((2, 0), (3, 1), (20, 18)):
        with pytest.raises(ValueError, match="stride"):
            DensePlan(LENGTHS, T, S, "mean", lookahead=L)
    for L in (-1, T, 2.0, True):
        with pytest.raises(ValueError, match="lookahead"):
            DensePlan(LENGTHS, T, 1, "mean", lookahead=L)
