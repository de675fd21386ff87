"""GPU: dense inference's blend in rotation space (csrc/blend_rot.hip) -- mmego_blend_rot, every frame's skeleton from the chordal mean
of the rotations the windows predicted for each bone, and the means themselves as quaternions -- against the float64 restatement of
tests/rot_blend_ref.py (SVD, where the kernel runs Jacobi sweeps on a 4 x 4 matrix), on synthetic rows.

Every source row is made on the host as the nets make one (rot_blend_ref.rigid_rows): per bone a base rotation times a perturbation of
at most 0.5 rad, a random proper head rotation, q = Rh G P, joints by forward kinematics, roots within 3 m (float64, one float32
rounding).  The restatement's smallest (lambda_1 - lambda_2) / W over the covers used here is asserted to be at least 1 (a single
rotation has 4): the top eigenvector is then at double rounding and no random cover takes the fallback.

Bounds: |out - ref| <= 2^-23 |ref| + 1e-7 on every element of dst, quat (after the canonical sign), spread and rot_spread
(dense_ref.within <= 1, the bound of the double-inside, float-store kernels); every blended bone within 2e-6 m of |body_b|, the margin of
two float-rounded endpoints at |coordinate| < 8 m (2 sqrt(3) 2^-24 8 = 1.7e-6; the coordinate range is asserted)."""
import numpy as np
import pytest
import torch

import bone_blend_ref as bref
import dense_ref as ref
import rot_blend_ref as rref

pytestmark = pytest.mark.gpu

SENT = -12345.0
NROWS = 120
TREES = {"upper": (15, rref.UPPER_WALK, rref.ROT_UPPER, 14), "lower": (8, rref.LOWER_WALK, rref.ROT_LOWER, 6)}
RIGID = 2e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _d(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _body(rng, nb):
    """A random bone set [nb, 3] with lengths in (0.05, 0.55) m."""
    u = rng.normal(size=(nb, 3))
    return (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.05, 0.55, (nb, 1))).astype(np.float32)


def _cover(rng, F):
    """Covers of 21, 2, 1 and 0 rows, frame after frame; weights the integers 1 .. 10."""
    counts = np.asarray([(21, 2, 1, 0)[f % 4] for f in range(F)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    row = rng.integers(0, NROWS, int(off[-1])).astype(np.int32)
    w = rng.integers(1, 11, len(row)).astype(np.float32)
    return off, row, w


def _raw(dev, rows, cover, tree, body, pad=0, extras=True):
    """The entry point itself (no host check of the cover, so that a row outside the source reaches the kernel).  Outputs are filled with
    sentinels and one row longer than F."""
    from mmego_amd import hip
    J, bones, rot_idx, NQ = TREES[tree]
    src, q, Rh = rows
    off, row, w = cover
    F, NB = len(off) - 1, len(bones)
    dst = torch.full((F + 1, 3 * J + pad), SENT, dtype=torch.float32, device=dev)
    quat = torch.full((F + 1, NB, 4), SENT, dtype=torch.float32, device=dev)
    spr, rspr = (torch.full((F + 1,), SENT, dtype=torch.float32, device=dev) for _ in range(2))
    fb = torch.full((F + 1,), -7, dtype=torch.int32, device=dev)
    hip.call("blend_rot", _d(dev, src), len(src), J, _d(dev, q), NQ, _d(dev, Rh), _d(dev, off), _d(dev, row), _d(dev, w), F,
             _d(dev, np.asarray(bones, dtype=np.int32)), _d(dev, np.asarray(rot_idx, dtype=np.int32)), _d(dev, body), NB, dst, 3 * J + pad,
             quat, spr if extras else None, rspr if extras else None, fb if extras else None)
    return dst, quat, spr, rspr, fb


@pytest.mark.parametrize("F", [1, 4, 5, 67])
@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_blend_rot_against_the_restatement(dev, tree, F):
    J, bones, rot_idx, NQ = TREES[tree]
    NB = len(bones)
    rng = np.random.default_rng(100 * F + J)
    body = _body(rng, NB)
    rows = src, q, Rh = rref.rigid_rows(rng, NROWS, J, bones, rot_idx, NQ, body)
    off, row, w = cover = _cover(rng, F)
    row[3] = NROWS                                     # frame 0, 21 entries: one names the row behind the source and is skipped
    if F > 5:
        row[off[5]] = -1                               # frame 5, 2 entries: one valid entry is left, its row is copied
    gaps = []
    want, want_q, want_spr, want_rspr, want_fb = rref.blend_rot(src, q, Rh, off, row, w, bones, rot_idx, body, min_gap=gaps)
    assert min(gaps) >= 1.0 and not want_fb.any() and np.abs(src).max() < 8.0
    L = np.linalg.norm(body.astype(np.float64), axis=1)
    for pad in (0, 3):
        dst, quat, spr, rspr, fb = _raw(dev, rows, cover, tree, body, pad)
        out, qt, s, rs, n = (t.cpu().numpy() for t in (dst, quat, spr, rspr, fb))
        assert np.all(out[:F, 3 * J:] == SENT) and np.all(out[F] == SENT) and np.all(qt[F] == SENT) and s[F] == SENT and rs[F] == SENT \
            and n[F] == -7, "written outside the F rows"
        assert not np.isnan(out).any() and not np.isnan(qt).any() and not np.isnan(s).any() and not np.isnan(rs).any()
        worst = ref.within(out[:F, :3 * J], want)
        worst_q = ref.within(rref.canonical(qt[:F]), want_q)
        worst_s, worst_r = ref.within(s[:F], want_spr), ref.within(rs[:F], want_rspr)
        print("%s F %d ldd 3J+%d: worst error / bound %.3f (dst) %.3f (quat) %.3f (spread) %.3f (rot_spread); rot_spread up to %.3f rad"
              % (tree, F, pad, worst, worst_q, worst_s, worst_r, want_rspr.max()))
        assert worst <= 1.0 and worst_q <= 1.0 and worst_s <= 1.0 and worst_r <= 1.0, (pad, worst, worst_q, worst_s, worst_r)
        assert not n[:F].any()
        # the stored quaternions are canonical already, and unit up to their float rounding
        covered = np.flatnonzero([any(0 <= r < NROWS for r in row[off[f]:off[f + 1]]) for f in range(F)])
        assert np.array_equal(rref.canonical(qt[covered]), qt[covered].astype(np.float64))
        assert np.abs(np.linalg.norm(qt[covered].astype(np.float64), axis=2) - 1.0).max() <= 2e-7
        empty = np.setdiff1d(np.arange(F), covered)
        assert not out[empty, :3 * J].any() and not qt[empty].any() and not s[empty].any() and not rs[empty].any(), \
            "an empty list gives a zero row, zero quaternions and spreads 0"
        # every blended bone has its rest length
        many = np.flatnonzero(np.diff(off) >= 2)
        if len(many):
            assert np.abs(out[:F, :3 * J]).max() < 8.0
            assert np.abs(bref.bone_lengths(out[many, :3 * J], bones) - L).max() <= RIGID
        # frames with one valid entry: the row, bit for bit, that entry's quaternion, no rotational spread
        once = [f for f in range(F) if off[f + 1] - off[f] == 1] + ([5] if F > 5 else [])
        for f in once:
            r = [int(x) for x in row[off[f]:off[f + 1]] if 0 <= x < NROWS]
            assert len(r) == 1 and np.array_equal(out[f, :3 * J], src[r[0]]) and s[f] == 0.0 and rs[f] == 0.0, f
        # two launches, the same bits
        again = _raw(dev, rows, cover, tree, body, pad)
        assert all(torch.equal(a, b) for a, b in zip((dst, quat, spr, rspr, fb), again))


@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_without_the_optional_outputs_the_same_bits(dev, tree):
    J, bones, rot_idx, NQ = TREES[tree]
    rng = np.random.default_rng(31 + J)
    body = _body(rng, len(bones))
    rows = rref.rigid_rows(rng, NROWS, J, bones, rot_idx, NQ, body)
    cover = _cover(rng, 67)
    dst, quat, spr, rspr, fb = _raw(dev, rows, cover, tree, body)
    dst2, quat2, spr2, rspr2, fb2 = _raw(dev, rows, cover, tree, body, extras=False)
    assert torch.equal(dst, dst2) and torch.equal(quat, quat2)
    assert bool((spr2 == SENT).all()) and bool((rspr2 == SENT).all()) and bool((fb2 == -7).all())
    assert not bool((spr[:67] == SENT).any()) and not bool((rspr[:67] == SENT).any()) and not bool((fb[:67] == -7).any())


def test_opposed_rotations_take_the_heaviest_window(dev):
    """The neck (bone 0 of the upper walk, rotation 3) is seen as the identity in row 0 and as a half turn about z in row 1, world frame
    (Rh = I in both).  At equal weights their sum is diag(0, 0, 2 w): the two largest eigenvalues meet, the mean has no direction -- the
    bone takes the FIRST entry's rotation and the frame counts one fallback, whichever row comes first; at weights 2 : 3 the heavier row
    wins and nothing is counted.  Every other bone of those frames, and every other frame, is blended as usual."""
    from mmego_amd import ops
    J, bones, rot_idx, NQ = TREES["upper"]
    rng = np.random.default_rng(11)
    body = _body(rng, 14)
    src, q, Rh = rref.rigid_rows(rng, NROWS, J, bones, rot_idx, NQ, body)
    half = np.diag([-1.0, -1.0, 1.0]).astype(np.float32)
    # rows 0 and 1: Rh = I, so q is the world rotation; every bone but the neck as row 2 sees it, the same in both rows
    world2 = (Rh[2].reshape(3, 3).T.astype(np.float64) @ q[2].reshape(14, 3, 3).astype(np.float64)).reshape(14, 9).astype(np.float32)
    for r, m in ((0, np.eye(3, dtype=np.float32)), (1, half)):
        Rh[r] = np.eye(3, dtype=np.float32).ravel()
        q[r] = world2
        q[r, 3] = m.ravel()
    off = np.array([0, 2, 4, 6, 6, 9], np.int64)
    row = np.array([0, 1, 1, 0, 0, 1, 30, 31, 32], np.int32)
    w = np.array([4, 4, 4, 4, 2, 3, 1, 5, 2], np.float32)
    F = 5
    dst = torch.full((F, 45), SENT, dtype=torch.float32, device=dev)
    quat = torch.full((F, 14, 4), SENT, dtype=torch.float32, device=dev)
    spr, rspr = (torch.full((F,), SENT, dtype=torch.float32, device=dev) for _ in range(2))
    fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
    ops.blend_rot(_d(dev, src), _d(dev, q), _d(dev, Rh), (off, row, w), bones, rot_idx, body, dst, quat, spr, rspr, fb)
    out, qt, n = dst.cpu().numpy(), quat.cpu().numpy(), fb.cpu().numpy()
    want, want_q, want_spr, want_rspr, want_fb = rref.blend_rot(src, q, Rh, off, row, w, bones, rot_idx, body)
    assert want_fb.tolist() == [1, 1, 0, 0, 0] and n.tolist() == [1, 1, 0, 0, 0]
    assert qt[0, 0].tolist() == [1, 0, 0, 0] and qt[1, 0].tolist() == [0, 0, 0, 1] and np.allclose(qt[2, 0], [0, 0, 0, 1], rtol=0, atol=1e-7)
    assert ref.within(out, want) <= 1.0 and ref.within(rref.canonical(qt), want_q) <= 1.0
    assert ref.within(spr.cpu().numpy(), want_spr) <= 1.0 and ref.within(rspr.cpu().numpy(), want_rspr) <= 1.0
    L = np.linalg.norm(body.astype(np.float64), axis=1)
    assert np.abs(out).max() < 8.0 and np.abs(bref.bone_lengths(out[[0, 1, 2, 4]], bones) - L).max() <= RIGID
    # the neck of frame 0 is the rest bone itself, of frame 1 its half turn about z, laid from the blended head (slot 14 -> slot 3)
    head = out[:2, 42:45].astype(np.float64)
    b0 = body[0].astype(np.float64)
    assert np.abs(out[0, 9:12] - (head[0] + b0)).max() <= 1e-6 and np.abs(out[1, 9:12] - (head[1] + b0 * [-1, -1, 1])).max() <= 1e-6


def test_refusals_leave_the_outputs_alone(dev):
    from mmego_amd import hip, ops
    J, bones, rot_idx, NQ = TREES["upper"]
    rng = np.random.default_rng(5)
    body = _body(rng, 14)
    F = 5
    src, q, Rh = (_d(dev, a) for a in rref.rigid_rows(rng, NROWS, J, bones, rot_idx, NQ, body))
    cover = _cover(rng, F)
    dst = torch.full((F, 45), SENT, dtype=torch.float32, device=dev)
    quat = torch.full((F, 14, 4), SENT, dtype=torch.float32, device=dev)
    spr, rspr = (torch.full((F,), SENT, dtype=torch.float32, device=dev) for _ in range(2))
    fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
    twice = [list(b) for b in bones]
    twice[5] = [3, 4]                                                  # joint 3 is bone 0's child already
    late = [list(b) for b in bones]
    late[0], late[1] = late[1], late[0]                                # (2, 3) ahead of (3, 14): the parent comes after its child
    zero, nan = body.copy(), body.copy()
    zero[4], nan[9, 1] = 0.0, np.nan
    far = list(rot_idx)
    far[2] = 14

    def call(**change):
        a = dict(src=src, q=q, Rh=Rh, cover=cover, bones=bones, rot_idx=rot_idx, body=body, dst=dst, quat=quat, spread=spr,
                 rot_spread=rspr, fallback=fb)
        a.update(change)
        return ops.blend_rot(**a)

    for what, change in (("a child listed twice", dict(bones=twice)), ("a parent after its child", dict(bones=late)),
                         ("a zero rest bone", dict(body=zero)), ("a NaN rest bone", dict(body=nan)),
                         ("a rotation outside a row's", dict(rot_idx=far)), ("a negative rotation", dict(rot_idx=[-1] + list(rot_idx[1:]))),
                         ("one rotation index too few", dict(rot_idx=rot_idx[:-1])), ("one rest bone too few", dict(body=body[:-1])),
                         ("a short dst", dict(dst=dst[:, :44])), ("a dst of other frames", dict(dst=dst[:4])),
                         ("a quat of other bones", dict(quat=quat[:, :13].contiguous())), ("a strided quat", dict(quat=quat[:, :, :2])),
                         ("q of other rows", dict(q=q[:-1])), ("a strided q", dict(q=q[:, :, :6])), ("Rh of other rows", dict(Rh=Rh[:-1])),
                         ("a double q", dict(q=q.double())), ("a host Rh", dict(Rh=Rh.cpu())),
                         ("a float fallback", dict(fallback=spr)), ("a short rot_spread", dict(rot_spread=rspr[:4])),
                         ("a cover of rows outside", dict(cover=(cover[0], np.where(cover[1] == cover[1][0], NROWS, cover[1]).astype(np.int32),
                                                                 cover[2])))):
        with pytest.raises((ValueError, IndexError, TypeError)):
            call(**change)
        torch.cuda.synchronize()
        assert bool((dst == SENT).all()) and bool((quat == SENT).all()) and bool((spr == SENT).all()) and bool((rspr == SENT).all()) \
            and bool((fb == -7).all()), what
    # the entry point itself
    off, row, w = (_d(dev, a) for a in cover)
    bd, rd, bod = _d(dev, np.asarray(bones, dtype=np.int32)), _d(dev, np.asarray(rot_idx, dtype=np.int32)), _d(dev, body)
    good = dict(src=src, nrows=NROWS, J=J, q=q, NQ=NQ, Rh=Rh, cov_off=off, cov_row=row, cov_w=w, F=F, bones=bd, rot_idx=rd, body=bod, NB=14,
                dst=dst, ldd=45, quat=quat, spread=spr, rot_spread=rspr, fallback=fb)
    for change in (dict(src=None), dict(q=None), dict(Rh=None), dict(cov_off=None), dict(cov_row=None), dict(cov_w=None), dict(dst=None),
                   dict(quat=None), dict(bones=None), dict(rot_idx=None), dict(body=None), dict(F=0), dict(J=1), dict(J=22, ldd=66),
                   dict(NB=15), dict(NB=0), dict(NQ=0), dict(NQ=65), dict(ldd=44), dict(quat=quat.view(-1)[1:])):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("blend_rot", *[a[k] for k in good])
    torch.cuda.synchronize()
    assert bool((dst == SENT).all()) and bool((quat == SENT).all()) and bool((spr == SENT).all()) and bool((fb == -7).all())
    call()                                                             # (and the good call goes through)
    assert not bool((dst == SENT).any()) and not bool((fb == -7).any())
    covered = torch.as_tensor(np.diff(cover[0]) > 0).to(dev)
    assert not bool((quat[covered] == SENT).any())
