"""GPU: the temporal filter of dense inference in its bone-direction form (csrc/smooth.hip, mmego_smooth_bones) with both walk tables,
against the float64 restatement of tests/smooth_ref.py, on rigid skeletons that move slowly: a root that drifts 2 cm a frame and bone
directions that turn by about a hundredth of a radian a frame, made on the host in float64 and rounded once.  Such rows stay far from the
fallback for every order (checked: the restatement counts none).

Bounds: |out - ref| <= 2^-23 |ref| + 1e-7 on every element of dst and moved (dense_ref.within <= 1); every filtered bone within 2e-6 m of
L_b, the bound tests/test_bone_blend_gpu.py holds mmego_blend_bones to (two float-rounded endpoints at |coordinate| < 8 m: 2 sqrt(3)
2^-24 8 = 1.7e-6; the coordinate range is asserted)."""
import numpy as np
import pytest
import torch

import bone_blend_ref as bref
import dense_ref as ref
import smooth_ref as sref
from test_smooth_gpu import DS, HS, SENT, TABLES, layout, table

pytestmark = pytest.mark.gpu

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
    u = rng.normal(size=(nb, 3))
    body = (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.05, 0.55, (nb, 1))).astype(np.float32)
    return body, np.linalg.norm(body.astype(np.float64), axis=1).astype(np.float32)


def slow_rows(rng, F, J, bones, L):
    """F rigid rows [F, 3 J] (float32) of a skeleton whose roots start within 2 m and drift, and whose bones turn slowly."""
    children = [c for c, _ in bones]
    roots = {j: rng.uniform(-2.0, 2.0, 3) for j in range(J) if j not in children}
    dirs = rng.normal(size=(len(bones), 3))
    rows = np.zeros((F, J, 3))
    for f in range(F):
        for j in roots:
            roots[j] = roots[j] + rng.normal(0.0, 0.02, 3)
            rows[f, j] = roots[j]
        dirs = dirs + rng.normal(0.0, 0.01, dirs.shape)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        for (c, p), d, l in zip(bones, dirs, L):
            rows[f, c] = rows[f, p] + float(l) * d
    return rows.reshape(F, 3 * J).astype(np.float32)


def _raw(dev, src, seg, w, D, J, bones, L, pad_s=0, pad_d=0, moved=True, fallback=True):
    from mmego_amd import hip
    F, C = src.shape
    wide = np.full((F, C + pad_s), 777.0, np.float32)
    wide[:, :C] = src
    dst = torch.full((F + 1, C + pad_d), SENT, dtype=torch.float32, device=dev)
    mv = torch.full((F + 1,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((F + 1,), -7, dtype=torch.int32, device=dev)
    hip.call("smooth_bones", _d(dev, wide), C + pad_s, F, J, _d(dev, seg), _d(dev, w), len(w) // 2, D,
             _d(dev, np.asarray(bones, dtype=np.int32)), _d(dev, L), len(bones), dst, C + pad_d, mv if moved else None,
             fb if fallback else None)
    return dst, mv, fb


@pytest.mark.parametrize("F", [1, 3, 65, 257])
@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_smooth_bones_against_the_restatement(dev, tree, F):
    from mmego_amd import hip
    J, bones = TREES[tree]
    C = 3 * J
    rng = np.random.default_rng(100 * F + J)
    _, L = _body(rng, len(bones))
    src = slow_rows(rng, F, J, bones, L)
    assert np.abs(src).max() < 8.0
    roots = [j for j in range(J) if j not in [c for c, _ in bones]]
    cols = [3 * j + i for j in roots for i in range(3)]
    worst, worst_m, worst_len, case = 0.0, 0.0, 0.0, 0
    for whole in ((False, True) if F == 3 else (False,)):
        seg = layout(F, whole)
        for H in HS:
            for D in DS:
                kind = TABLES[(case + (H > 1)) % 3]                      # (the three tables take turns over the nine (H, D))
                w = table(rng, H, kind)
                want, want_m, want_fb = sref.smooth_bones(src, seg, w, D, bones, L)
                assert not want_fb.any()
                case += 1
                pad_s, pad_d = (0, 0) if case % 2 else (3, 5)
                dst, mv, fb = _raw(dev, src, seg, w, D, J, bones, L, pad_s, pad_d)
                out, m, n = dst.cpu().numpy(), mv.cpu().numpy(), fb.cpu().numpy()
                assert np.all(out[:F, C:] == SENT) and np.all(out[F] == SENT) and m[F] == SENT and n[F] == -7, "written outside the F rows"
                assert not np.isnan(out).any() and not n[:F].any() and np.abs(out[:F, :C]).max() < 8.0
                worst, worst_m = max(worst, ref.within(out[:F, :C], want)), max(worst_m, ref.within(m[:F], want_m))
                worst_len = max(worst_len, np.abs(bref.bone_lengths(out[:F, :C], bones) - L.astype(np.float64)).max())
                # frames outside every segment, or alone in their own: the row, bit for bit
                alone = np.asarray([len(sref.valid_taps(seg, f, H)) <= 1 for f in range(F)])
                assert np.array_equal(out[:F, :C][alone], src[alone]) and not m[:F][alone].any(), (H, D, kind)
                # the roots: the column form's bits
                plain = torch.full((F, C), SENT, dtype=torch.float32, device=dev)
                hip.call("smooth_frames", _d(dev, src), C, F, C, _d(dev, seg), _d(dev, w), H, D, plain, C, None)
                assert torch.equal(dst[:F, cols], plain[:, cols]), (H, D, kind)
                # two launches, the same bits; without moved and fallback the same dst, those buffers untouched
                dst2, mv2, fb2 = _raw(dev, src, seg, w, D, J, bones, L, pad_s, pad_d)
                assert torch.equal(dst, dst2) and torch.equal(mv, mv2) and torch.equal(fb, fb2)
                dst3, mv3, fb3 = _raw(dev, src, seg, w, D, J, bones, L, pad_s, pad_d, moved=False, fallback=False)
                assert torch.equal(dst, dst3) and bool((mv3 == SENT).all()) and bool((fb3 == -7).all())
    print("%s F %d: worst error / bound %.3f (dst) %.3f (moved), worst | |bone| - L | %.3e m over %d launches" % (
        tree, F, worst, worst_m, worst_len, case))
    assert worst <= 1.0 and worst_m <= 1.0 and worst_len <= RIGID


def test_the_column_form_shortens_bones_and_the_bones_form_does_not(dev):
    """Through ops, with the project's walk tables: a skeleton whose bones turn by a tenth of a radian a frame, under a wide moving
    average.  The column filter shortens the bones by centimetres; the bones form keeps them."""
    from mmego_amd import dense, ops, skeleton
    rng = np.random.default_rng(17)
    for walk, J in ((skeleton.WALK_UPPER, 15), (skeleton.WALK_LOWER, 8)):
        bones = [tuple(b) for b in walk.tolist()]
        _, L = _body(rng, len(bones))
        F = 70
        src = slow_rows(rng, F, J, bones, L)
        fast = src.astype(np.float64).reshape(F, J, 3).copy()          # the same roots, bones that turn ten times as fast
        dirs = rng.normal(size=(len(bones), 3))
        for f in range(F):
            dirs = dirs + rng.normal(0.0, 0.1, dirs.shape)
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            for (c, p), d, l in zip(bones, dirs, L):
                fast[f, c] = fast[f, p] + float(l) * d
        srcd = _d(dev, fast.reshape(F, 3 * J).astype(np.float32))
        seg = np.zeros(F, np.int32)
        w = dense.smooth_weights(8, "gauss")
        rigid, plain = (torch.full((F, 3 * J), SENT, dtype=torch.float32, device=dev) for _ in range(2))
        fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
        ops.smooth_bones(srcd, seg, w, 0, walk, L, rigid, None, fb)
        ops.smooth_frames(srcd, seg, w, 0, plain)
        dev_rigid = np.abs(bref.bone_lengths(rigid.cpu().numpy(), bones) - L.astype(np.float64)).max()
        dev_plain = np.abs(bref.bone_lengths(plain.cpu().numpy(), bones) - L.astype(np.float64)).max()
        print("J %d: worst | |bone| - L | %.3e m bones form, %.3e m column form" % (J, dev_rigid, dev_plain))
        assert np.abs(rigid.cpu().numpy()).max() < 8.0
        assert dev_rigid <= RIGID and dev_plain > 1e-2 and not fb.cpu().numpy().any()
        want, _, _ = sref.smooth_bones(fast.reshape(F, 3 * J).astype(np.float32), seg, w, 0, bones, L)
        assert ref.within(rigid.cpu().numpy(), want) <= 1.0


def test_a_bone_that_reverses_between_two_frames_keeps_its_own_direction(dev):
    """Two frames of one segment under D = 0 and the box taper of H = 1: both frames weigh their two valid taps 1 / 2 each.  The neck
    bone (bone 0 of the upper walk: head 14 -> joint 3, L = 0.25) points along +x in frame 0 and -x in frame 1, from heads at multiples
    of 0.25, so the filtered vector is exactly zero: each frame keeps its own direction from the filtered head, counts one fallback, and
    the joints below stay rigid."""
    from mmego_amd import dense, ops
    J, bones = TREES["upper"]
    rng = np.random.default_rng(11)
    body, _ = _body(rng, len(bones))
    body[0] = (0.0, 0.25, 0.0)
    L = np.linalg.norm(body.astype(np.float64), axis=1).astype(np.float32)
    a = bref.rigid_row(rng, J, bones, body, roots={14: np.asarray((0.5, -0.75, 1.25))}, dirs={0: (1.0, 0.0, 0.0)})
    b = a.copy()
    b[14] = (1.0, -0.5, 1.25)
    b[3] = b[14] + (-0.25, 0.0, 0.0)
    for c, p in bones[1:]:
        b[c] = b[p] + (a[c] - a[p])
    src = np.stack([a.ravel(), b.ravel()]).astype(np.float32)
    assert np.array_equal(src[0, 9:12] - src[0, 42:45], [0.25, 0, 0]) and np.array_equal(src[1, 9:12] - src[1, 42:45], [-0.25, 0, 0])
    seg = np.array([4, 4], np.int32)
    w = dense.smooth_weights(1, "box")
    dst = torch.full((2, 45), SENT, dtype=torch.float32, device=dev)
    mv = torch.full((2,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((2,), -7, dtype=torch.int32, device=dev)
    ops.smooth_bones(_d(dev, src), seg, w, 0, bones, L, dst, mv, fb)
    out = dst.cpu().numpy()
    want, want_m, want_fb = sref.smooth_bones(src, seg, w, 0, bones, L)
    assert fb.cpu().numpy().tolist() == [1, 1] and want_fb.tolist() == [1, 1]
    assert ref.within(out, want) <= 1.0 and ref.within(mv.cpu().numpy(), want_m) <= 1.0
    head = np.array([0.75, -0.625, 1.25])
    for f, x in ((0, 0.25), (1, -0.25)):
        assert np.array_equal(out[f, 42:45].astype(np.float64), head) and np.array_equal(out[f, 9:12].astype(np.float64), head + [x, 0.0, 0.0])
    assert np.abs(bref.bone_lengths(out, bones) - L.astype(np.float64)).max() <= RIGID and np.abs(out).max() < 8.0
    # with the second frame in a segment of its own nothing is filtered: both rows bit for bit, no fallback
    ops.smooth_bones(_d(dev, src), np.array([4, -1], np.int32), w, 0, bones, L, dst, mv, fb)
    assert np.array_equal(dst.cpu().numpy(), src) and not mv.cpu().numpy().any() and not fb.cpu().numpy().any()


def test_refusals_leave_the_outputs_alone(dev):
    from mmego_amd import dense, hip, ops
    J, bones = TREES["upper"]
    rng = np.random.default_rng(5)
    _, L = _body(rng, len(bones))
    F = 9
    src = _d(dev, slow_rows(rng, F, J, bones, L))
    seg = np.zeros(F, np.int32)
    w = dense.smooth_weights(2, "gauss")
    dst = torch.full((F, 45), SENT, dtype=torch.float32, device=dev)
    mv = torch.full((F,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
    twice = [list(b) for b in bones]
    twice[5] = [3, 4]                                                  # joint 3 is bone 0's child already
    late = [list(b) for b in bones]
    late[0], late[1] = late[1], late[0]                                # (2, 3) ahead of (3, 14): the parent comes after its child
    zero = L.copy()
    zero[4] = 0.0
    for what, call in (("a child listed twice", lambda: ops.smooth_bones(src, seg, w, 2, twice, L, dst, mv, fb)),
                       ("a parent after its child", lambda: ops.smooth_bones(src, seg, w, 2, late, L, dst, mv, fb)),
                       ("a zero length", lambda: ops.smooth_bones(src, seg, w, 2, bones, zero, dst, mv, fb)),
                       ("one length too few", lambda: ops.smooth_bones(src, seg, w, 2, bones, L[:-1], dst, mv, fb)),
                       ("rows that are no 3-vectors", lambda: ops.smooth_bones(src[:, :44], seg, w, 2, bones, L, dst, mv, fb)),
                       ("dst is src", lambda: ops.smooth_bones(src, seg, w, 2, bones, L, src, mv, fb)),
                       ("an even weight length", lambda: ops.smooth_bones(src, seg, w[:-1], 2, bones, L, dst, mv, fb)),
                       ("order 3", lambda: ops.smooth_bones(src, seg, w, 3, bones, L, dst, mv, fb)),
                       ("a short seg", lambda: ops.smooth_bones(src, seg[:-1], w, 2, bones, L, dst, mv, fb)),
                       ("a float fallback", lambda: ops.smooth_bones(src, seg, w, 2, bones, L, dst, mv, mv))):
        with pytest.raises((ValueError, IndexError)):
            call()
        torch.cuda.synchronize()
        assert bool((dst == SENT).all()) and bool((mv == SENT).all()) and bool((fb == -7).all()), what
    segd, wd = _d(dev, seg), _d(dev, w)
    bd, ld = _d(dev, np.asarray(bones, dtype=np.int32)), _d(dev, L)
    good = dict(src=src, lds=45, F=F, J=J, seg=segd, w=wd, H=2, D=2, bones=bd, bone_len=ld, NB=14, dst=dst, ldd=45, moved=mv, fallback=fb)
    for change in (dict(src=None), dict(seg=None), dict(w=None), dict(dst=None), dict(F=0), dict(J=0), dict(J=22, lds=66, ldd=66),
                   dict(NB=15), dict(NB=-1), dict(bones=None), dict(bone_len=None), dict(lds=44), dict(ldd=44), dict(H=0), dict(H=32),
                   dict(D=3), dict(dst=src)):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("smooth_bones", *[a[k] for k in good])
    torch.cuda.synchronize()
    assert bool((dst == SENT).all()) and bool((mv == SENT).all()) and bool((fb == -7).all())
    ops.smooth_bones(src, seg, w, 2, bones, L, dst, mv, fb)            # (and the good call goes through)
    assert not bool((dst == SENT).any()) and not bool((fb == -7).any())
