"""GPU: mmego_pose_jitter (csrc/pose_noise.hip) -- every frame's head pose perturbed by a random rotation and shift drawn from a device
seed word -- against the numpy restatement of its recipe (tests/pose_noise_ref.py), on properties that do not lean on the restatement,
on the statistics of the recovered draws, inside a replayed HIP graph, and on what the launcher refuses."""
import numpy as np
import pytest
import torch

import pose_noise_ref as pref
from dense_ref import within

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORDS = (0, 1, 2 ** 63 - 1)
SIGMAS = ((1.0, 0.0), (0.0, 0.02), (3.0, 0.05), (1e-6, 0.0))                      # (the last takes the series branch)
NS = (1, 63, 64, 65, 257, 1000)


def _poses(n, seed=0):
    """R [n, 3, 3] random rotations from QR (determinant +1), t [n, 3] ~ N(0, 1), as fp32."""
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return q.astype(np.float32), rs.standard_normal((n, 3)).astype(np.float32)


def _word(w):
    return torch.tensor([w], dtype=torch.int64, device=DEV)


def _launch(R, t, sigma_deg, sigma_t, word, ids=None, inplace=False):
    from mmego_amd import ops
    Rd, td = torch.as_tensor(R).to(DEV), torch.as_tensor(t).to(DEV)
    Ro = Rd if inplace else torch.full_like(Rd, float("nan"))                      # (every entry has to be written)
    to = td if inplace else torch.full_like(td, float("nan"))
    ops.pose_jitter(Rd, td, sigma_deg, sigma_t, word if isinstance(word, torch.Tensor) else _word(word), Ro, to,
                    ids=None if ids is None else torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(DEV))
    return Ro.cpu().numpy(), to.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ids(n):
    """A permutation of the row numbers with repeats: a third of the rows take another row's draw number."""
    rs = np.random.RandomState(n)
    ids = rs.permutation(n).astype(np.int64)
    ids[rs.random_sample(n) < 1.0 / 3.0] = ids[0]
    return ids


@pytest.mark.parametrize("sigmas", SIGMAS)
@pytest.mark.parametrize("n", NS)
def test_against_the_restatement(n, sigmas):
    R, t = _poses(n, seed=n)
    worst = 0.0
    for word in WORDS:
        for ids in (None, _ids(n)):
            Ro, to = _launch(R, t, sigmas[0], sigmas[1], word, ids)
            Rw, tw = pref.pose_jitter(R, t, sigmas[0], sigmas[1], word, ids)
            assert not np.isnan(Ro).any() and not np.isnan(to).any()
            worst = max(worst, within(Ro, Rw), within(to, tw))
    print("n %d sigmas %s: worst error %.3f of 2^-23 |ref| + 1e-7" % (n, sigmas, worst))
    assert worst <= 1.0


def test_properties_without_the_restatement():
    n = 257
    R, t = _poses(n, seed=3)
    full = _launch(R, t, 3.0, 0.05, 7)
    again = _launch(R, t, 3.0, 0.05, 7)
    other = _launch(R, t, 3.0, 0.05, 8)
    for a, b, c in zip(full, again, other):
        assert np.array_equal(_bits(a), _bits(b)), "the same word: the same bytes"
        assert (_bits(a) != _bits(c)).mean() > 0.9, "another word: other bytes"
    # sigma_deg = 0: R is copied, t is the full launch's; sigma_t = 0: the mirror image
    R0 = R.copy()
    R0[::5, 0, 1] = -0.0                                                           # (a copy keeps the sign of a zero; E R would not)
    t0 = t.copy()
    t0[::7, 2] = -0.0
    Ro, to = _launch(R0, t, 0.0, 0.05, 7)
    assert np.array_equal(_bits(Ro), _bits(R0)) and np.array_equal(_bits(to), _bits(full[1]))
    Ro, to = _launch(R, t0, 3.0, 0.0, 7)
    assert np.array_equal(_bits(Ro), _bits(full[0])) and np.array_equal(_bits(to), _bits(t0))
    # aliased outputs equal disjoint outputs
    Ri, ti = _launch(R, t, 3.0, 0.05, 7, inplace=True)
    assert np.array_equal(_bits(Ri), _bits(full[0])) and np.array_equal(_bits(ti), _bits(full[1]))
    # rows with equal ids and equal inputs get equal outputs; rows with other ids do not
    ids = np.array([5, 9, 5, 2 ** 40 + 5, 9, 5, 11], dtype=np.int64)               # (the draw number is the id's low 32 bits)
    Rs, ts = np.repeat(R[:1], len(ids), axis=0), np.repeat(t[:1], len(ids), axis=0)
    Ro, to = _launch(Rs, ts, 3.0, 0.05, 7, ids)
    for a in (Ro.reshape(len(ids), -1), to):
        assert np.array_equal(_bits(a[0]), _bits(a[2])) and np.array_equal(_bits(a[0]), _bits(a[5])) and np.array_equal(_bits(a[1]), _bits(a[4]))
        assert np.array_equal(_bits(a[0]), _bits(a[3]))
        assert not np.array_equal(_bits(a[0]), _bits(a[1])) and not np.array_equal(_bits(a[0]), _bits(a[6]))
    # the output is a rotation: every entry within about 8e-8 of an exact rotation's (its own rounding plus the input's), so the Gram
    # error is about 3e-7
    for sd in (1.0, 3.0, 1e-6):
        Ro = _launch(R, t, sd, 0.0, 7)[0].astype(np.float64)
        gram = np.abs(Ro @ Ro.transpose(0, 2, 1) - np.eye(3)).max()
        print("sigma_deg %g: |R R^T - I| <= %.3g" % (sd, gram))
        assert gram <= 1e-6
        assert (np.linalg.det(Ro) > 0.999).all()


def test_statistics_of_the_recovered_draws():
    n, sd, st = 65536, 1.0, 0.02
    R, t = _poses(n, seed=5)
    Ro, to = _launch(R, t, sd, st, 12345678901234567)
    E = Ro.astype(np.float64) @ R.astype(np.float64).transpose(0, 2, 1)
    w = np.degrees(pref.rotation_vectors(E)) / sd                                   # in units of sigma
    dt = (to.astype(np.float64) - t.astype(np.float64)) / st
    # R and R_out are fp32: w is recovered to about 1e-5 sigma at 1 degree, dt to about 6e-6 sigma at 2 cm
    for name, v in (("rotation", w), ("translation", dt)):
        N = v.size
        mean, var, big = abs(v.mean()), abs(v.var() - 1.0), np.abs(v).max()
        print("%s: |mean| %.4f (bound %.4f), |var - 1| %.4f (bound %.4f), max |z| %.4f" % (
            name, mean, 5 / np.sqrt(N), var, 5 * np.sqrt(1.7 / N), big))
        assert big <= 3.4642
        assert mean <= 5 / np.sqrt(N)
        assert var <= 5 * np.sqrt(1.7 / N)                                         # (1.7: the kurtosis 2.7 of a sum of four uniforms, less 1)
    c = np.corrcoef(np.concatenate([w, dt], axis=1).T)
    off = np.abs(c - np.eye(6)).max()
    print("largest off-diagonal correlation of the six channels: %.4f (bound %.4f)" % (off, 4 / np.sqrt(n)))
    assert off < 4 / np.sqrt(n)


def test_captured_launch_follows_the_word():
    """One captured launch, replayed three times with the word rewritten in between, equals three eager launches bit for bit."""
    from mmego_amd import ops
    n = 300
    R, t = _poses(n, seed=9)
    Rd, td = torch.as_tensor(R).to(DEV), torch.as_tensor(t).to(DEV)
    Ro, to, word = torch.zeros_like(Rd), torch.zeros_like(td), _word(0)
    ops.pose_jitter(Rd, td, 2.0, 0.03, word, Ro, to)                                # (warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.capture(g):
        ops.pose_jitter(Rd, td, 2.0, 0.03, word, Ro, to)
    for key in (11, 2 ** 62 + 3, 11):
        word.fill_(key)
        g.replay()
        torch.cuda.synchronize()
        Re, te = _launch(R, t, 2.0, 0.03, key)
        assert np.array_equal(_bits(Ro.cpu().numpy()), _bits(Re)) and np.array_equal(_bits(to.cpu().numpy()), _bits(te)), key


def test_launcher_refusals():
    """Non-zero return, nothing launched: the outputs keep their fill."""
    from mmego_amd import hip
    n = 8
    R, t = _poses(n)
    buf = torch.zeros(64 * n, dtype=torch.float32, device=DEV)                     # one allocation to cut overlapping views from
    Rd, td = buf[n:10 * n], buf[16 * n:19 * n]
    Rd.copy_(torch.as_tensor(R).reshape(-1)), td.copy_(torch.as_tensor(t).reshape(-1))
    Ro, to = buf[32 * n:41 * n], buf[48 * n:51 * n]
    Ro.fill_(3.0), to.fill_(3.0)
    word = torch.zeros(4, dtype=torch.int64, device=DEV)
    ids = torch.arange(n + 1, dtype=torch.int64, device=DEV)
    fn = hip.lib().mmego_pose_jitter
    st = hip.stream_handle()
    ok = [st, Rd.data_ptr(), td.data_ptr(), n, 1.0, 0.02, word.data_ptr(), ids.data_ptr(), Ro.data_ptr(), to.data_ptr()]
    bad_sigma = (-1.0, float("nan"), float("inf"), float("-inf"))
    cases = [(1, None), (2, None), (8, None), (9, None), (6, None), (3, 0), (3, -1)]
    cases += [(4, s) for s in bad_sigma] + [(5, s) for s in bad_sigma]
    cases += [(6, word.data_ptr() + 4), (7, ids.data_ptr() + 4)]                   # not 8-byte aligned
    cases += [(8, Rd.data_ptr() + 36), (8, Rd.data_ptr() - 4), (9, td.data_ptr() + 12), (9, td.data_ptr() + 4)]      # shifted over their inputs
    cases += [(9, Ro.data_ptr() + 36 * n - 4), (9, Ro.data_ptr()), (8, td.data_ptr()), (9, Rd.data_ptr() + 12)]      # R_out / t_out, and across
    for pos, bad in cases:
        args = list(ok)
        args[pos] = bad
        assert fn(*args) != 0, (pos, bad)
    args = list(ok)
    args[4] = args[5] = 0.0                                                         # both sigmas zero: nothing to draw
    assert fn(*args) != 0
    torch.cuda.synchronize()
    assert bool((Ro == 3.0).all()) and bool((to == 3.0).all())
    assert bool((Rd.cpu() == torch.as_tensor(R).reshape(-1)).all())        # (a refused in-place overlap wrote nothing either)
    assert fn(*ok) == 0
    inplace = list(ok)
    inplace[8], inplace[9] = Rd.data_ptr(), td.data_ptr()                           # exactly in place: allowed
    assert fn(*inplace) == 0
    torch.cuda.synchronize()
    assert not bool((Ro == 3.0).any()) and not bool((to == 3.0).any())
    assert torch.equal(Ro, Rd) and torch.equal(to, td)
