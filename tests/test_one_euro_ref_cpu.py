"""CPU: the numpy restatement of the causal filter (tests/one_euro_ref.py) by a second route -- with beta = 0 the recursion is a plain
exponential filter with a closed form -- its exact properties (a constant run, causality), and ops.one_euro_runs on hand-made segments."""
import numpy as np
import pytest

import one_euro_ref as oref


def test_alpha():
    assert oref.alpha(1.0 / (2.0 * np.pi)) == pytest.approx(0.5, abs=1e-15)
    a = oref.alpha(np.array([0.02, 0.1, 5.0]))
    assert np.allclose(a, [0.111635, 0.385870, 0.969151], atol=1e-5) and (np.diff(a) > 0).all()


@pytest.mark.parametrize("fc", [0.02, 0.1, 5.0])
def test_beta_0_is_the_closed_form(fc):
    """xhat_i = (1 - a)^i x_0 + sum_{k < i} a (1 - a)^k x_{i-k}, whatever the speed estimate's cutoff."""
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 0.7, (40, 5, 3))
    a = float(oref.alpha(fc))
    want = np.empty_like(x)
    for i in range(len(x)):
        want[i] = (1.0 - a) ** i * x[0] + sum(a * (1.0 - a) ** k * x[i - k] for k in range(i))
    for dc in (0.1, 2.0):
        assert np.abs(oref.filter_vectors(x, fc, 0.0, dc) - want).max() <= 1e-12


@pytest.mark.parametrize("beta", [0.0, 40.0])
def test_a_constant_run_comes_back_exactly(beta):
    x = np.tile(np.random.default_rng(5).normal(0.0, 0.7, (1, 15, 3)).astype(np.float32).astype(np.float64), (30, 1, 1))
    assert np.array_equal(oref.filter_vectors(x, 0.05, beta, 0.1), x)
    src = x.reshape(30, 45)
    dst, moved = oref.one_euro(src, oref.runs_of(np.zeros(30, np.int32)), 0.05, beta, 0.1)
    assert np.array_equal(dst, src) and (moved == 0.0).all()


def test_a_frame_does_not_depend_on_later_frames():
    rng = np.random.default_rng(7)
    x = rng.normal(0.0, 0.7, (50, 15, 3))
    y = oref.filter_vectors(x, 0.05, 10.0, 0.1)
    for cut in (1, 2, 17, 49):
        z = x.copy()
        z[cut:] = rng.normal(0.0, 0.7, z[cut:].shape)
        assert np.array_equal(oref.filter_vectors(z, 0.05, 10.0, 0.1)[:cut], y[:cut]), cut
        assert not np.array_equal(oref.filter_vectors(z, 0.05, 10.0, 0.1)[cut], y[cut])


def test_the_cutoff_rises_with_speed_and_ignores_the_axes():
    """A ramp is followed more closely with beta > 0; rotating the input rotates the output (one cutoff per joint, not per coordinate)."""
    x = np.linspace(0.0, 3.0, 60)[:, None, None] * np.array([[[1.0, 2.0, -0.5]]])
    lag0 = np.abs(oref.filter_vectors(x, 0.02, 0.0, 0.1) - x)[-1].max()
    lag1 = np.abs(oref.filter_vectors(x, 0.02, 40.0, 0.1) - x)[-1].max()
    assert lag1 < 0.2 * lag0
    rng = np.random.default_rng(9)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    z = rng.normal(0.0, 0.7, (30, 4, 3))
    assert np.abs(oref.filter_vectors(z @ q.T, 0.05, 10.0, 0.1) - oref.filter_vectors(z, 0.05, 10.0, 0.1) @ q.T).max() <= 1e-12


SEGS = [([-1, -1, 0, 0, 0, -1, 1, 1, -1], [0, 2, 5, 6, 8, 9], [0, 1, 0, 1, 0]),          # gaps at head, middle and tail
        ([0, 0, 1, 1, 1, 3], [0, 2, 5, 6], [1, 1, 1]),                                    # adjacent recordings
        ([4], [0, 1], [1]), ([-1], [0, 1], [0]),                                          # F = 1
        ([2, 2, 2, 2], [0, 4], [1]), ([-1, -1, -1], [0, 3], [0])]


@pytest.mark.parametrize("seg,off,on", SEGS)
def test_one_euro_runs(seg, off, on):
    from mmego_amd import ops
    run_off, run_on = ops.one_euro_runs(np.asarray(seg, np.int32))
    assert run_off.dtype == np.int64 and run_on.dtype == np.int32
    assert run_off.tolist() == off and run_on.tolist() == on
    ref_off, ref_on = oref.runs_of(np.asarray(seg, np.int32))
    assert np.array_equal(run_off, ref_off) and np.array_equal(run_on, ref_on)
    assert run_off[0] == 0 and run_off[-1] == len(seg) and (np.diff(run_off) >= 1).all()       # a partition: one owner per row


def test_one_euro_runs_refuses_other_inputs():
    from mmego_amd import ops
    for bad in (np.zeros(4, np.int64), np.zeros((2, 2), np.int32), np.zeros(0, np.int32)):
        with pytest.raises(ValueError, match="one_euro_runs"):
            ops.one_euro_runs(bad)
