"""GPU: the bone-length-preserving blend of dense inference (csrc/blend_bones.hip) -- mmego_blend_bones, every frame's skeleton from the
window rows that cover it with every bone kept at the body's length, and mmego_bone_length_dev, the table of deviations from those
lengths -- against the float64 restatement of tests/bone_blend_ref.py, on synthetic rows.

Every source row is a rigid skeleton made on the host: random rotations applied to a random bone set, roots within 3 m (float64, one
float32 rounding).  Checked on the CPU: such rows deviate from their bone lengths by 2.4e-7 m, the restated blend stored as float32 by
3.6e-7 m at coordinates up to 5.2 m, and the smallest |s| / (W L) over 2 000 random covers was 0.04 -- random rows never take the fallback.

Bounds: |out - ref| <= 2^-23 |ref| + 1e-7 on every element of dst and spread (dense_ref.within <= 1, the bound of the double-inside,
float-store kernels); every blended bone within 2e-6 m of L_b, the margin of two float-rounded endpoints at |coordinate| < 8 m
(2 sqrt(3) 2^-24 8 = 1.7e-6; the coordinate range is asserted)."""
import numpy as np
import pytest
import torch

import bone_blend_ref as bref
import dense_ref as ref

pytestmark = pytest.mark.gpu

SENT = -12345.0
NROWS = 120
TREES = {"upper": (15, bref.UPPER_WALK), "lower": (8, bref.LOWER_WALK)}
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
    """A random bone set [nb, 3] with lengths in (0.05, 0.55) m, and L_b = float32(|body_b|) as dense.bone_lengths takes it."""
    u = rng.normal(size=(nb, 3))
    body = (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.05, 0.55, (nb, 1))).astype(np.float32)
    return body, np.linalg.norm(body.astype(np.float64), axis=1).astype(np.float32)


def _cover(rng, F):
    """Covers of 21, 2, 1 and 0 rows, frame after frame; weights the integers 1 .. 10."""
    counts = np.asarray([(21, 2, 1, 0)[f % 4] for f in range(F)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    row = rng.integers(0, NROWS, int(off[-1])).astype(np.int32)
    w = rng.integers(1, 11, len(row)).astype(np.float32)
    return off, row, w


def _raw(dev, src, cover, J, bones, L, pad=0, spread=True, fallback=True):
    """The entry point itself (no host check of the cover, so that a row outside the source reaches the kernel)."""
    from mmego_amd import hip
    off, row, w = cover
    F = len(off) - 1
    dst = torch.full((F + 1, 3 * J + pad), SENT, dtype=torch.float32, device=dev)          # (one more row behind the last: it stays)
    spr = torch.full((F + 1,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((F + 1,), -7, dtype=torch.int32, device=dev)
    hip.call("blend_bones", _d(dev, src), len(src), J, _d(dev, off), _d(dev, row), _d(dev, w), F,
             _d(dev, np.asarray(bones, dtype=np.int32)), _d(dev, L), len(bones), dst, 3 * J + pad, spr if spread else None,
             fb if fallback else None)
    return dst, spr, fb


@pytest.mark.parametrize("F", [1, 4, 5, 67])
@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_blend_bones_against_the_restatement(dev, tree, F):
    J, bones = TREES[tree]
    rng = np.random.default_rng(100 * F + J)
    body, L = _body(rng, len(bones))
    src = bref.rigid_rows(rng, NROWS, J, bones, body)
    off, row, w = cover = _cover(rng, F)
    row[3] = NROWS                                     # frame 0, 21 entries: one names the row behind the source and is skipped
    if F > 5:
        row[off[5]] = -1                               # frame 5, 2 entries: one valid entry is left, its row is copied
    want, want_spr, want_fb = bref.blend_bones(src, off, row, w, bones, L)
    assert not want_fb.any()
    for pad in (0, 3):
        dst, spr, fb = _raw(dev, src, cover, J, bones, L, pad)
        out, s, n = dst.cpu().numpy(), spr.cpu().numpy(), fb.cpu().numpy()
        assert np.all(out[:F, 3 * J:] == SENT) and np.all(out[F] == SENT) and s[F] == SENT and n[F] == -7, "written outside the F rows"
        worst, worst_s = ref.within(out[:F, :3 * J], want), ref.within(s[:F], want_spr)
        print("%s F %d ldd 3J+%d: worst error / bound %.3f (dst) %.3f (spread)" % (tree, F, pad, worst, worst_s))
        assert worst <= 1.0 and worst_s <= 1.0, (pad, worst, worst_s)
        assert not np.isnan(out).any() and not np.isnan(s).any() and not n[:F].any()
        empty = np.flatnonzero(np.diff(off) == 0)
        assert not out[empty, :3 * J].any() and not s[empty].any(), "an empty list gives a zero row and spread 0"
        # frames with one valid entry: the row, bit for bit
        once = [f for f in range(F) if off[f + 1] - off[f] == 1] + ([5] if F > 5 else [])
        for f in once:
            r = [int(x) for x in row[off[f]:off[f + 1]] if 0 <= x < NROWS]
            assert len(r) == 1 and np.array_equal(out[f, :3 * J], src[r[0]]) and s[f] == 0.0, f
        # two launches, the same bits
        dst2, spr2, fb2 = _raw(dev, src, cover, J, bones, L, pad)
        assert torch.equal(dst, dst2) and torch.equal(spr, spr2) and torch.equal(fb, fb2)
    # without spread and fallback: the same dst, those buffers untouched
    dst3, spr3, fb3 = _raw(dev, src, cover, J, bones, L, 0, spread=False, fallback=False)
    assert torch.equal(dst3, _raw(dev, src, cover, J, bones, L, 0)[0]) and bool((spr3 == SENT).all()) and bool((fb3 == -7).all())


@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_blended_bones_keep_their_length_and_roots_their_bits(dev, tree):
    from mmego_amd import ops
    J, bones = TREES[tree]
    rng = np.random.default_rng(7 + J)
    body, L = _body(rng, len(bones))
    src = bref.rigid_rows(rng, NROWS, J, bones, body)
    F = 67
    off, row, w = cover = _cover(rng, F)
    srcd = _d(dev, src)
    dst = torch.full((F, 3 * J), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
    ops.blend_bones(srcd, cover, bones, L, dst, None, fb)
    out = dst.cpu().numpy()
    assert np.abs(out).max() < 8.0 and np.abs(src).max() < 8.0
    many = np.flatnonzero(np.diff(off) >= 2)
    assert len(many) >= 30
    dev_rigid = np.abs(bref.bone_lengths(out[many], bones) - L.astype(np.float64)).max()
    plain = torch.full((F, 3 * J), SENT, dtype=torch.float32, device=dev)
    ops.blend_windows(srcd, cover, plain)
    dev_plain = np.abs(bref.bone_lengths(plain.cpu().numpy()[many], bones) - L.astype(np.float64)).max()
    print("%s: worst | |bone| - L | %.3e m rigid, %.3e m under the vector mean" % (tree, dev_rigid, dev_plain))
    assert dev_rigid <= RIGID and dev_plain > 1e-2
    assert not fb.cpu().numpy().any()
    # the roots are the vector mean's columns, bit for bit; a frame covered once is its row
    roots = [j for j in range(J) if j not in [c for c, _ in bones]]
    assert len(roots) == (1 if tree == "upper" else 2)
    cols = [3 * j + i for j in roots for i in range(3)]
    assert torch.equal(dst[:, cols], plain[:, cols])
    once = np.flatnonzero(np.diff(off) == 1)
    assert len(once) >= 10 and np.array_equal(out[once], src[row[off[once]]])


def test_a_forearm_seen_90_degrees_apart_keeps_its_length(dev):
    """Two equal-weight windows that agree on everything but the forearm's direction (bone 6 of the upper walk, elbow 5 -> wrist 6; the
    hand follows): the vector mean makes the forearm L / sqrt(2), the bone blend L."""
    from mmego_amd import ops
    J, bones = TREES["upper"]
    rng = np.random.default_rng(90)
    body, L = _body(rng, len(bones))
    a = bref.rigid_rows(rng, 1, J, bones, body)[0].astype(np.float64).reshape(J, 3)
    b = a.copy()
    da = (a[6] - a[5]) / np.linalg.norm(a[6] - a[5])
    db = np.cross(da, [0.3, -0.5, 0.8])
    db /= np.linalg.norm(db)
    assert abs(da @ db) < 1e-15
    b[6] = b[5] + np.linalg.norm(body[6].astype(np.float64)) * db
    b[7] = b[6] + (a[7] - a[6])
    src = np.stack([a.ravel(), b.ravel()]).astype(np.float32)
    cover = (np.array([0, 2], np.int64), np.array([0, 1], np.int32), np.array([3.0, 3.0], np.float32))
    rigid, plain = (torch.full((1, 45), SENT, dtype=torch.float32, device=dev) for _ in range(2))
    ops.blend_bones(_d(dev, src), cover, bones, L, rigid)
    ops.blend_windows(_d(dev, src), cover, plain)
    lr, lp = bref.bone_lengths(rigid.cpu().numpy(), bones)[0], bref.bone_lengths(plain.cpu().numpy(), bones)[0]
    print("forearm: L %.7f, vector mean %.7f (L / sqrt 2 = %.7f), bone blend %.7f" % (L[6], lp[6], L[6] / np.sqrt(2.0), lr[6]))
    assert abs(lp[6] - float(L[6]) / np.sqrt(2.0)) <= 1e-6
    assert np.abs(lr - L.astype(np.float64)).max() <= RIGID


def test_a_cancelled_bone_takes_the_heaviest_window(dev):
    """Frame 2 of 5: two equal-weight entries whose neck bone (bone 0 of the upper walk: head 14 -> joint 3) has exactly opposite
    differences, +-0.25 along x from a head at multiples of 0.25, so that the weighted sum is exactly zero.  The bone takes the first
    entry's direction, the frame counts one fallback, the joints below stay rigid; no other frame counts one."""
    from mmego_amd import ops
    J, bones = TREES["upper"]
    rng = np.random.default_rng(11)
    body, _ = _body(rng, len(bones))
    body[0] = (0.0, 0.25, 0.0)
    L = np.linalg.norm(body.astype(np.float64), axis=1).astype(np.float32)
    src = bref.rigid_rows(rng, NROWS, J, bones, body)
    for r, (head, x) in enumerate((((0.5, -0.75, 1.25), 1.0), ((0.75, -0.5, 1.25), -1.0))):
        src[r] = bref.rigid_row(rng, J, bones, body, roots={14: np.asarray(head)}, dirs={0: (x, 0.0, 0.0)}).ravel().astype(np.float32)
    assert np.array_equal(src[0, 9:12] - src[0, 42:45], [0.25, 0, 0]) and np.array_equal(src[1, 9:12] - src[1, 42:45], [-0.25, 0, 0])
    off = np.array([0, 2, 5, 7, 7, 8], np.int64)
    row = np.array([5, 9, 30, 31, 32, 0, 1, 77], np.int32)
    w = np.array([1, 2, 3, 3, 1, 4, 4, 2], np.float32)
    F = 5
    dst = torch.full((F, 45), SENT, dtype=torch.float32, device=dev)
    spr = torch.full((F,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
    ops.blend_bones(_d(dev, src), (off, row, w), bones, L, dst, spr, fb)
    out, n = dst.cpu().numpy(), fb.cpu().numpy()
    assert n.tolist() == [0, 0, 1, 0, 0]
    want, want_spr, want_fb = bref.blend_bones(src, off, row, w, bones, L)
    assert want_fb.tolist() == [0, 0, 1, 0, 0]
    assert ref.within(out, want) <= 1.0 and ref.within(spr.cpu().numpy(), want_spr) <= 1.0
    head = out[2, 42:45].astype(np.float64)
    assert np.array_equal(head, [0.625, -0.625, 1.25]) and np.array_equal(out[2, 9:12], head + [0.25, 0.0, 0.0])
    assert np.abs(bref.bone_lengths(out[[0, 1, 2]], bones) - L.astype(np.float64)).max() <= RIGID
    assert np.abs(out).max() < 8.0


def test_refusals_leave_the_outputs_alone(dev):
    from mmego_amd import hip, ops
    J, bones = TREES["upper"]
    rng = np.random.default_rng(5)
    body, L = _body(rng, len(bones))
    F = 5
    src = _d(dev, bref.rigid_rows(rng, NROWS, J, bones, body))
    cover = _cover(rng, F)
    dst = torch.full((F, 45), SENT, dtype=torch.float32, device=dev)
    spr = torch.full((F,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
    twice = [list(b) for b in bones]
    twice[5] = [3, 4]                                                  # joint 3 is bone 0's child already
    late = [list(b) for b in bones]
    late[0], late[1] = late[1], late[0]                                # (2, 3) ahead of (3, 14): the parent comes after its child
    zero, nan = L.copy(), L.copy()
    zero[4], nan[9] = 0.0, np.nan
    wide = torch.zeros((NROWS, 66), dtype=torch.float32, device=dev)   # J = 22
    wide_bones = [(j + 1, j) for j in range(21)]
    for what, call in (("a child listed twice", lambda: ops.blend_bones(src, cover, twice, L, dst, spr, fb)),
                       ("a parent after its child", lambda: ops.blend_bones(src, cover, late, L, dst, spr, fb)),
                       ("22 joints", lambda: ops.blend_bones(wide, cover, wide_bones, np.ones(21, np.float32), dst, spr, fb)),
                       ("a zero length", lambda: ops.blend_bones(src, cover, bones, zero, dst, spr, fb)),
                       ("a NaN length", lambda: ops.blend_bones(src, cover, bones, nan, dst, spr, fb)),
                       ("a short dst", lambda: ops.blend_bones(src, cover, bones, L, dst[:, :44], spr, fb)),
                       ("a dst of other frames", lambda: ops.blend_bones(src, cover, bones, L, dst[:4], spr, fb)),
                       ("one length too few", lambda: ops.blend_bones(src, cover, bones, L[:-1], dst, spr, fb)),
                       ("a float fallback", lambda: ops.blend_bones(src, cover, bones, L, dst, spr, spr))):
        with pytest.raises((ValueError, IndexError, TypeError)):
            call()
        torch.cuda.synchronize()
        assert bool((dst == SENT).all()) and bool((spr == SENT).all()) and bool((fb == -7).all()), what
    # the entry points themselves
    off, row, w = (_d(dev, a) for a in cover)
    bd, ld = _d(dev, np.asarray(bones, dtype=np.int32)), _d(dev, L)
    good = dict(src=src, nrows=NROWS, J=J, cov_off=off, cov_row=row, cov_w=w, F=F, bones=bd, bone_len=ld, NB=14, dst=dst, ldd=45,
                spread=spr, fallback=fb)
    for change in (dict(src=None), dict(cov_off=None), dict(cov_row=None), dict(cov_w=None), dict(dst=None), dict(F=0), dict(J=0),
                   dict(J=22, ldd=66), dict(NB=15), dict(NB=-1), dict(bones=None), dict(bone_len=None), dict(ldd=44)):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("blend_bones", *[a[k] for k in good])
    out = torch.full((F, 14), SENT, dtype=torch.float32, device=dev)
    good2 = dict(X=src, ldx=45, n=F, J=J, bones=bd, bone_len=ld, NB=14, out=out, ldo=14)
    for change in (dict(X=None), dict(bones=None), dict(bone_len=None), dict(out=None), dict(n=0), dict(J=22), dict(NB=0), dict(NB=15),
                   dict(ldx=44), dict(ldo=13)):
        a = dict(good2, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("bone_length_dev", *[a[k] for k in good2])
    torch.cuda.synchronize()
    assert bool((dst == SENT).all()) and bool((spr == SENT).all()) and bool((fb == -7).all()) and bool((out == SENT).all())
    ops.blend_bones(src, cover, bones, L, dst, spr, fb)                # (and the good call goes through)
    assert not bool((dst == SENT).any()) and not bool((fb == -7).any())


@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_bone_length_dev_against_the_restatement(dev, tree, n):
    from mmego_amd import ops
    J, bones = TREES[tree]
    NB = len(bones)
    rng = np.random.default_rng(n + J)
    body, L = _body(rng, NB)
    X = bref.rigid_rows(rng, n, J, bones, body) + rng.normal(0.0, 0.02, (n, 3 * J)).astype(np.float32)     # (rows that do deviate)
    want = bref.bone_length_dev(X, bones, L)
    for pad in (0, 5):
        Xd = _d(dev, np.concatenate([X, np.zeros((n, pad), np.float32)], axis=1))
        out = torch.full((n + 1, NB + 2), SENT, dtype=torch.float32, device=dev)
        ops.bone_length_dev(Xd[:, :3 * J], bones, L, out[:n, :NB])
        got = out.cpu().numpy()
        assert np.all(got[:n, NB:] == SENT) and np.all(got[n] == SENT)
        worst = ref.within(got[:n, :NB], want)
        print("%s n %d ldx 3J+%d: worst error / bound %.3f" % (tree, n, pad, worst))
        assert worst <= 1.0 and want.max() > 1e-3
