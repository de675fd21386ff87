"""GPU: mmego_imu_jitter (csrc/imu_noise.hip) -- every IMU sample perturbed by white noise of its own and by its window's bias, drawn
from a device seed word -- against the numpy restatement of its recipe (tests/imu_noise_ref.py), on properties that do not lean on the
restatement, on the statistics of the recovered draws, inside a replayed HIP graph, and on what the launcher and ops.imu_jitter refuse."""
import numpy as np
import pytest
import torch

import imu_noise_ref as iref
from dense_ref import within

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORDS = (1, 2 ** 63 - 12345)                                                       # (the second: bits above 32 set)
ALL_SIX = (1.0, 0.05, 0.01, 2.0, 0.2, 0.02)
SIGMAS = tuple(tuple(ALL_SIX[k] if k == j else 0.0 for k in range(6)) for j in range(6)) + (
    ALL_SIX[:3] + (0.0,) * 3, (0.0,) * 3 + ALL_SIX[3:], ALL_SIX)                  # each alone, white only, bias only, all six
# (n_rows, T, S): the smallest; one window; several; 260 samples, past one 256-thread workgroup; S = 1 and S = 3
SHAPES = ((1, 1, 20), (3, 3, 20), (12, 4, 20), (13, 1, 20), (20, 5, 1), (20, 5, 3))
GRID_CAP = 2048 * 256                                                              # sample-threads of one launch; beyond: the strided loop
STRIDED = (GRID_CAP // 20 + 1, 5, 20)                                              # 26 215 rows: the smallest n_rows past the cap (31 MB)


def _samples(n_rows, S, seed=0):
    """imu [n_rows, S, 15] fp32: a random rotation from QR (determinant +1), accelerometer ~ 3 N(0, 1), gyroscope ~ N(0, 1); some zeros
    carry a minus sign (a copy keeps it)."""
    rs = np.random.RandomState(seed)
    n = n_rows * S
    q, r = np.linalg.qr(rs.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    x = np.concatenate([q.reshape(n, 9), 3.0 * rs.standard_normal((n, 3)), rs.standard_normal((n, 3))], axis=1).astype(np.float32)
    x[::5, :9] = np.array([-0.0, 1, -0.0, -1, 0, -0.0, 0, -0.0, 1], dtype=np.float32)      # (a quarter turn about z: exact, signed zeros)
    x[::7, 10] = x[::3, 14] = -0.0
    return x.reshape(n_rows, S, 15)


def _word(w):
    return torch.tensor([w], dtype=torch.int64, device=DEV)


def _dev_ids(ids):
    return None if ids is None else torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(DEV)


def _launch(imu, T, sigmas, word, row_ids=None, win_ids=None, inplace=False):
    from mmego_amd import ops
    x = torch.as_tensor(imu).to(DEV)
    out = x if inplace else torch.full_like(x, float("nan"))                       # (every entry has to be written)
    got = ops.imu_jitter(x, sigmas, word if isinstance(word, torch.Tensor) else _word(word), out, T=T, row_ids=_dev_ids(row_ids),
                         win_ids=_dev_ids(win_ids))
    assert got is out
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ids(n, seed):
    """A permutation of 0 .. n-1 with repeats: a third of the entries take the first one's number."""
    rs = np.random.RandomState(seed)
    ids = rs.permutation(n).astype(np.int64)
    ids[rs.random_sample(n) < 1.0 / 3.0] = ids[0]
    return ids


def _check(imu, T, sigmas, word, row_ids, win_ids):
    """One launch against the restatement -> the worst error in units of the bound; groups whose sigmas are 0 are the input's bits."""
    out = _launch(imu, T, sigmas, word, row_ids, win_ids)
    want = iref.imu_jitter(imu, T, sigmas, word, row_ids, win_ids)
    assert not np.isnan(out).any()
    for lo, hi, a, b in ((0, 9, 0, 3), (9, 12, 1, 4), (12, 15, 2, 5)):
        if sigmas[a] == 0 and sigmas[b] == 0:
            assert np.array_equal(_bits(out[..., lo:hi]), _bits(imu[..., lo:hi])), (lo, sigmas)
        else:
            assert (_bits(out[..., lo:hi]) != _bits(imu[..., lo:hi])).mean() > 0.5, (lo, sigmas)
    return within(out, want)


@pytest.mark.parametrize("sigmas", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_restatement(shape, sigmas):
    n_rows, T, S = shape
    imu = _samples(n_rows, S, seed=n_rows + S)
    worst = 0.0
    for word in WORDS:
        for row_ids, win_ids in ((None, None), (_ids(n_rows, 1), None), (None, _ids(n_rows // T, 2)), (_ids(n_rows, 3), _ids(n_rows // T, 4))):
            worst = max(worst, _check(imu, T, sigmas, word, row_ids, win_ids))
    print("shape %s sigmas %s: worst error %.3f of 2^-23 |ref| + 1e-7" % (shape, sigmas, worst))
    assert worst <= 1.0


def test_the_strided_loop_against_the_restatement():
    """The launcher caps its grid at 2048 workgroups of 256: the smallest input whose last samples are a thread's SECOND."""
    n_rows, T, S = STRIDED
    assert (n_rows - 1) * S <= GRID_CAP < n_rows * S and n_rows % T == 0
    rs = np.random.RandomState(11)
    imu = np.tile(_samples(n_rows // T, S, seed=11), (T, 1, 1))                    # (a fifth of the rotations made, then repeated)
    imu[..., 9:] += rs.standard_normal((n_rows, S, 6)).astype(np.float32)
    worst = _check(imu, T, ALL_SIX, WORDS[1], _ids(n_rows, 5), _ids(n_rows // T, 6))
    print("%d rows, %d samples: worst error %.3f of 2^-23 |ref| + 1e-7" % (n_rows, n_rows * S, worst))
    assert worst <= 1.0


def test_properties_without_the_restatement():
    n_rows, T, S = 24, 4, 20
    imu = _samples(n_rows, S, seed=3)
    full = _launch(imu, T, ALL_SIX, 7)
    assert np.array_equal(_bits(full), _bits(_launch(imu, T, ALL_SIX, 7))), "the same word: the same bytes"
    assert (_bits(full) != _bits(_launch(imu, T, ALL_SIX, 8))).mean() > 0.9, "another word: other bytes"
    assert np.array_equal(_bits(_launch(imu, T, ALL_SIX, 7, inplace=True)), _bits(full)), "in place: the same bytes"
    # bias only: the offsets of a window's T S samples agree to one rounding (half an ulp of the output each), and differ between windows
    bias = (0.0,) * 3 + ALL_SIX[3:]
    out = _launch(imu, T, bias, 7).astype(np.float64)
    off = (out - imu.astype(np.float64))[..., 9:].reshape(n_rows // T, T * S, 6)
    spread = off.max(axis=1) - off.min(axis=1)
    ulp = 2.0 ** -23 * np.abs(out[..., 9:]).reshape(n_rows // T, T * S, 6).max(axis=1)
    assert (spread <= ulp + 1e-12).all(), (spread / ulp).max()                     # (1e-12: the double roundings inside)
    mean = off.mean(axis=1)
    assert (np.abs(mean[:, None] - mean[None])[~np.eye(len(mean), dtype=bool)] > 1e-6).all(), "windows draw their own bias"
    assert np.abs(mean[:, :3]).max() <= 3.47 * bias[4] and np.abs(mean[:, 3:]).max() <= 3.47 * bias[5]
    # and the orientations of a window are turned by ONE rotation: O' O^T is the same matrix for all its samples
    Ew = (out[..., :9].reshape(-1, 3, 3) @ imu[..., :9].astype(np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)).reshape(n_rows // T, T * S, 9)
    assert (Ew.max(axis=1) - Ew.min(axis=1)).max() <= 1e-6
    assert np.abs(Ew[0, 0] - Ew[1, 0]).max() > 1e-4
    # a frame given twice under one row_ids value, in two windows with different win_ids: the same white part.  White only: the same
    # bits; all six: what differs between the copies is the two windows' bias, constant over the frame's samples (the white part cancels)
    twice = np.concatenate([imu[:T], imu[:T]])
    row_ids, win_ids = np.array(list(range(100, 100 + T)) * 2), np.array([5, 9])
    white = _launch(twice, T, ALL_SIX[:3] + (0.0,) * 3, 7, row_ids, win_ids)
    assert np.array_equal(_bits(white[:T]), _bits(white[T:]))
    assert not np.array_equal(_bits(white[0]), _bits(white[1]))
    both = _launch(twice, T, ALL_SIX, 7, row_ids, win_ids).astype(np.float64)
    diff = (both[:T] - both[T:])[..., 9:].reshape(T * S, 6)
    assert (diff.max(axis=0) - diff.min(axis=0) <= 2.0 ** -22 * np.abs(both[..., 9:]).max()).all() and (np.abs(diff.mean(axis=0)) > 1e-6).all()
    same = _launch(twice, T, ALL_SIX, 7, row_ids, np.array([5, 2 ** 32 + 5]))      # (the draw number is the id's low 32 bits)
    assert np.array_equal(_bits(same[:T]), _bits(same[T:]))


def test_the_output_is_a_rotation():
    """10 degrees per axis on both factors, orthonormal fp32 inputs: the float64 arithmetic alone, rounded to fp32, leaves |O' O'^T - I| at
    about 1.7e-7 (an entry's own rounding plus the input's)."""
    n_rows, T, S = 64, 4, 20
    imu = _samples(n_rows, S, seed=5)
    for sig in ((10.0, 0, 0, 10.0, 0, 0), (10.0, 0, 0, 0, 0, 0), (0, 0, 0, 10.0, 0, 0), (1e-6, 0, 0, 1e-6, 0, 0)):
        O = _launch(imu, T, sig, 7)[..., :9].astype(np.float64).reshape(-1, 3, 3)
        gram = np.abs(O @ O.transpose(0, 2, 1) - np.eye(3)).max()
        print("sigmas %s: |O' O'^T - I| <= %.3g" % (sig, gram))
        assert gram <= 1e-6
        assert (np.linalg.det(O) > 0.999).all()
    # neither factor turns by more than 6 times its sigma: the angle of O' O^T under one factor
    for sig in ((10.0, 0, 0, 0, 0, 0), (0, 0, 0, 10.0, 0, 0)):
        O = _launch(imu, T, sig, 7)[..., :9].astype(np.float64).reshape(-1, 3, 3)
        E = O @ imu[..., :9].astype(np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)
        angle = np.degrees(np.arccos(np.clip(0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0), -1.0, 1.0)))
        assert 1.0 < angle.max() <= 6 * 10.0


def _stats(name, z):
    N = z.size
    mean, var, big = abs(z.mean()), abs(z.var() - 1.0), np.abs(z).max()
    print("%s: N %d, |mean| %.4f (bound %.4f), |var - 1| %.4f (bound %.4f), max |z| %.4f" % (
        name, N, mean, 5 / np.sqrt(N), var, 5 * np.sqrt(1.7 / N), big))
    assert N >= 2e5
    assert big <= 3.4642
    assert mean <= 5 / np.sqrt(N)
    assert var <= 5 * np.sqrt(1.7 / N)                                             # (1.7: the kurtosis 2.7 of a sum of four uniforms, less 1)


def test_statistics_of_the_recovered_draws():
    """The additive draws recovered as (out - in) / sigma; inputs within +-2, so that at sigma = 0.05 the output's rounding moves a
    recovered draw by no more than 2.4e-6."""
    rs = np.random.RandomState(6)
    sig = 0.05
    # white: 4096 rows of 20 samples, three channels a group
    imu = _samples(4096, 20, seed=6)
    imu[..., 9:] = rs.uniform(-2.0, 2.0, (4096, 20, 6)).astype(np.float32)
    out = _launch(imu, 4, (0, sig, sig, 0, 0, 0), 12345678901234567)
    z = (out.astype(np.float64) - imu.astype(np.float64))[..., 9:].reshape(-1, 6) / sig
    _stats("white, accelerometer", z[:, :3]), _stats("white, gyroscope", z[:, 3:])
    assert np.abs(np.corrcoef(z.T) - np.eye(6)).max() < 4 / np.sqrt(len(z))
    # bias: 70 000 windows of one frame of one sample
    imu = np.zeros((70000, 1, 15), dtype=np.float32)
    imu[..., 9:] = rs.uniform(-2.0, 2.0, (70000, 1, 6)).astype(np.float32)
    out = _launch(imu, 1, (0, 0, 0, 0, sig, sig), 12345678901234567)
    assert np.array_equal(_bits(out[..., :9]), _bits(imu[..., :9]))
    z = (out.astype(np.float64) - imu.astype(np.float64))[..., 9:].reshape(-1, 6) / sig
    _stats("bias, accelerometer", z[:, :3]), _stats("bias, gyroscope", z[:, 3:])
    assert np.abs(np.corrcoef(z.T) - np.eye(6)).max() < 4 / np.sqrt(len(z))


def test_captured_launch_follows_the_word():
    """One captured launch, replayed with the word rewritten in between, draws anew each time and equals the eager launch bit for bit;
    the same word gives the same bytes."""
    from mmego_amd import ops
    n_rows, T, S = 15, 3, 20
    imu = _samples(n_rows, S, seed=9)
    x = torch.as_tensor(imu).to(DEV)
    out, word = torch.zeros_like(x), _word(0)
    ops.imu_jitter(x, ALL_SIX, word, out, T=T)                                      # (warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.capture(g):
        ops.imu_jitter(x.view(-1, S, 15), ALL_SIX, word, out.view(-1, S, 15), T=T)
    seen = {}
    for key in (11, 2 ** 62 + 3, 11):
        word.fill_(key)
        g.replay()
        torch.cuda.synchronize()
        got = _bits(out.cpu().numpy())
        assert np.array_equal(got, _bits(_launch(imu, T, ALL_SIX, key))), key
        assert key not in seen or np.array_equal(seen[key], got)
        seen[key] = got
    assert (seen[11] != seen[2 ** 62 + 3]).mean() > 0.9
    assert torch.equal(x.cpu(), torch.as_tensor(imu)), "out of place: the input is never written"


def test_launcher_refusals():
    """Non-zero return, nothing launched: the output keeps its fill."""
    from mmego_amd import hip
    n_rows, T, S = 6, 3, 20
    n = n_rows * S * 15
    imu = _samples(n_rows, S)
    buf = torch.zeros(4 * n, dtype=torch.float32, device=DEV)                      # one allocation to cut overlapping views from
    x, out = buf[:n], buf[2 * n:3 * n]
    x.copy_(torch.as_tensor(imu).reshape(-1))
    out.fill_(3.0)
    word = torch.zeros(4, dtype=torch.int64, device=DEV)
    row_ids = torch.arange(n_rows + 1, dtype=torch.int64, device=DEV)
    win_ids = torch.arange(n_rows // T + 1, dtype=torch.int64, device=DEV)
    fn = hip.lib().mmego_imu_jitter
    ok = [hip.stream_handle(), x.data_ptr(), n_rows, T, S, 1.0, 0.05, 0.01, 2.0, 0.2, 0.02, word.data_ptr(), row_ids.data_ptr(),
          win_ids.data_ptr(), out.data_ptr()]
    cases = [(1, None), (14, None), (11, None)]                                    # a null imu, out, seed_word
    cases += [(2, 0), (2, -3), (3, 0), (3, -1), (4, 0), (4, -20), (3, 4), (2, 7)]  # n_rows, T, S below 1; n_rows no multiple of T
    cases += [(pos, s) for pos in range(5, 11) for s in (-1.0, float("nan"), float("inf"), float("-inf"))]
    cases += [(11, word.data_ptr() + 4), (12, row_ids.data_ptr() + 4), (13, win_ids.data_ptr() + 4)]      # not 8-byte aligned
    cases += [(14, x.data_ptr() + 60), (14, x.data_ptr() - 4), (14, x.data_ptr() + 4 * n - 4), (1, out.data_ptr() + 4)]      # shifted over the input
    for pos, bad in cases:
        args = list(ok)
        args[pos] = bad
        assert fn(*args) != 0, (pos, bad)
    args = list(ok)
    args[5:11] = [0.0] * 6                                                          # all six sigmas zero: nothing to draw
    assert fn(*args) != 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert bool((x.cpu() == torch.as_tensor(imu).reshape(-1)).all())               # (a refused in-place overlap wrote nothing either)
    assert bool((buf[n:2 * n] == 0).all()) and bool((buf[3 * n:] == 0).all())
    assert fn(*ok) == 0
    nulls = list(ok)
    nulls[12] = nulls[13] = None                                                    # null ids: allowed
    assert fn(*nulls) == 0
    inplace = list(nulls)
    inplace[14] = x.data_ptr()                                                      # exactly in place: allowed
    assert fn(*inplace) == 0
    torch.cuda.synchronize()
    assert not bool((out == 3.0).any())
    assert torch.equal(out, x)
    assert bool((buf[n:2 * n] == 0).all()) and bool((buf[3 * n:] == 0).all())      # nothing beside the two buffers was written


def test_ops_imu_jitter_refusals_on_the_device():
    """What tests/test_imu_noise_cli_cpu.py cannot reach without a device word: the ids."""
    from mmego_amd import ops
    x = torch.zeros(2, 3, 20, 15, device=DEV)
    out, word = torch.full_like(x, 3.0), _word(1)
    ids = lambda n, **kw: torch.arange(n, **dict(dict(dtype=torch.int64, device=DEV), **kw))
    for kw in (dict(row_ids=ids(6, device="cpu")), dict(row_ids=ids(6, dtype=torch.int32)), dict(win_ids=ids(4)[::2]), dict(win_ids=[0, 1])):
        with pytest.raises(TypeError, match="contiguous int64 draw numbers on the device"):
            ops.imu_jitter(x, ALL_SIX, word, out, **kw)
    for kw, said in ((dict(row_ids=ids(5)), "5 row_ids for 6 frames"), (dict(row_ids=ids(2)), "2 row_ids for 6 frames"),
                     (dict(win_ids=ids(6)), "6 win_ids for 2 windows"), (dict(win_ids=ids(3), T=1), "3 win_ids for 6 windows")):
        with pytest.raises(ValueError, match=said):
            ops.imu_jitter(x, ALL_SIX, word, out, **kw)
    with pytest.raises(TypeError):
        ops.imu_jitter(x.cpu(), ALL_SIX, word, out)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert ops.imu_jitter(x, ALL_SIX, word, out, T=2, row_ids=ids(6), win_ids=ids(3)) is out and not bool((out == 3.0).any())
