"""GPU: the temporal filter of dense inference in rotation space (csrc/smooth.hip, mmego_smooth_rot) with both walk tables, against the
float64 restatement of tests/rot_smooth_ref.py -- coefficients from a least-squares solve, the filtered rotation from numpy's eigh, where
the kernel has cofactors and Jacobi sweeps.

Inputs: per bone a random base rotation times, in every frame, a rotation of at most 0.6 rad about a random axis, as quaternions rounded to
float32 with a random sign each; roots N(0, 0.7); src's bone columns are the forward kinematics of those rotations.  The segment layout
is that of tests/test_smooth_gpu.py (a segment of one frame, one of two, uncovered frames, the 63 | 64 workgroup edge; at F = 3 also one
whole segment), H in {1, 3, 31}, D in {0, 1, 2}, the tables box / gauss / random in [0.5, 2]: all 27 at every F and tree.

Bound: |out - ref| <= 2^-23 |ref| + 1e-7 (dense_ref.within <= 1, the bound of the double-inside, float-store kernels) on dst, on quat_out
after rot_blend_ref.canonical, on moved and on rot_moved.  Worked out on the CPU (scripts/rot_smooth_host_check.hip, the kernel's
arithmetic lane by lane under the host sanitizers against long-double arithmetic with a polar iteration, on rows made the same way, the
same layout, all 27 (H, D, table) at F in {1, 3, 64, 65, 257}, both trees): worst error / bound 0.3504, largest sum |c_k| 2.2304, least
eigenvalue gap / sum |c_k| 1.685 (the fallback's threshold is 1e-9), worst bone length error 1.9e-7 m, no violation.  The test asserts
gap >= 1e-3 on its own inputs and no fallback.

Where the recipe's own clauses meet: a frame with n <= 1 valid taps copies its quaternions bit for bit, so ITS quat_out carries the
input's sign (not the canonical one) and follows a sign flip of the input; every other row has canonical sign and ignores the flip.
The designed fallback needs c = (1/2, 1/2) on two taps: that is order 0 (at order 1, 2 the degree falls to 1 and the line through two
taps, evaluated at one of them, is that tap: c = (1, 0))."""
import numpy as np
import pytest
import torch

import bone_blend_ref as bref
import dense_ref as ref
import rot_blend_ref as rref
import rot_smooth_ref as rsref
import smooth_ref as sref
from test_smooth_gpu import DS, HS, SENT, TABLES, layout, table

pytestmark = pytest.mark.gpu

TREES = {"upper": (15, bref.UPPER_WALK), "lower": (8, bref.LOWER_WALK)}
RIGID, UNIT, JOINT = 2e-6, 2e-7, 2e-5


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
    return (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.05, 0.55, (nb, 1))).astype(np.float32)


def _raw(dev, src, quat, seg, w, D, J, bones, body, pad_s=0, pad_d=0, moved=True, rot_moved=True, fallback=True):
    """The entry point itself on a source of row stride 3 J + pad_s, a dst of row stride 3 J + pad_d, one more row behind every output."""
    from mmego_amd import hip
    F, C = src.shape
    NB = len(bones)
    wide = np.full((F, C + pad_s), 777.0, np.float32)
    wide[:, :C] = src
    dst = torch.full((F + 1, C + pad_d), SENT, dtype=torch.float32, device=dev)
    qo = torch.full((F + 1, NB, 4), SENT, dtype=torch.float32, device=dev)
    mv, rm = (torch.full((F + 1,), SENT, dtype=torch.float32, device=dev) for _ in range(2))
    fb = torch.full((F + 1,), -7, dtype=torch.int32, device=dev)
    hip.call("smooth_rot", _d(dev, wide), C + pad_s, F, J, _d(dev, quat), NB, _d(dev, seg), _d(dev, w), len(w) // 2, D,
             _d(dev, np.asarray(bones, dtype=np.int32)), _d(dev, body), dst, C + pad_d, qo, mv if moved else None, rm if rot_moved else None,
             fb if fallback else None)
    return dst, qo, mv, rm, fb


def _fk(roots, quat, bones, body):
    """numpy forward kinematics [n, 3 J] of stored quaternions [n, NB, 4] over body from the root joints of the rows ``roots``."""
    pos = np.array(roots, dtype=np.float64).reshape(len(roots), -1, 3)
    Q = rsref.matrices(quat)
    for b, (c, p) in enumerate(bones):
        pos[:, c] = pos[:, p] + Q[:, b] @ np.asarray(body[b], dtype=np.float64)
    return pos.reshape(len(roots), -1)


def _canonical_sign(q):
    lead = np.where(q[..., 0] != 0, q[..., 0], np.where(q[..., 1] != 0, q[..., 1], np.where(q[..., 2] != 0, q[..., 2], q[..., 3])))
    return bool((lead > 0).all())


@pytest.mark.parametrize("F", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_smooth_rot_against_the_restatement(dev, tree, F):
    from mmego_amd import hip
    J, bones = TREES[tree]
    C, NB = 3 * J, len(bones)
    rng = np.random.default_rng(100 * F + J)
    body = _body(rng, NB)
    L = np.linalg.norm(body.astype(np.float64), axis=1)
    src, quat, _, _ = rsref.rows_of(rng, rsref.jittery_rotations(rng, F, NB, 0.6), bones, body, J)
    assert np.abs(src).max() < 8.0
    roots = [j for j in range(J) if j not in [c for c, _ in bones]]
    cols = [3 * j + i for j in roots for i in range(3)]
    flip = np.where(rng.random((F, NB, 1)) < 0.5, -1.0, 1.0).astype(np.float32)
    other = rsref.rows_of(rng, rsref.jittery_rotations(rng, F, NB, 0.6), bones, body, J)      # what the frames outside a segment are rewritten with
    worst = dict(dst=0.0, quat=0.0, moved=0.0, rot_moved=0.0, length=0.0, unit=0.0, fk=0.0)
    gaps, sums, case = [], [], 0
    for whole in ((False, True) if F == 3 else (False,)):
        seg = layout(F, whole)
        inside = seg == seg[F - 1] if seg[F - 1] >= 0 else np.zeros(F, bool)          # the last frame's segment
        for H in HS:
            alone = np.asarray([len(sref.valid_taps(seg, f, H)) <= 1 for f in range(F)])
            for D in DS:
                for kind in TABLES:
                    w = table(rng, H, kind)
                    want, want_q, want_m, want_r, want_fb = rsref.smooth_rot(src, quat, seg, w, D, bones, body, min_gap=gaps, sum_abs=sums)
                    assert not want_fb.any()
                    case += 1
                    pad_s, pad_d = (0, 0) if case % 2 else (3, 5)
                    dst, qo, mv, rm, fb = _raw(dev, src, quat, seg, w, D, J, bones, body, pad_s, pad_d)
                    out, q, m, r, n = dst.cpu().numpy(), qo.cpu().numpy(), mv.cpu().numpy(), rm.cpu().numpy(), fb.cpu().numpy()
                    assert np.all(out[:F, C:] == SENT) and np.all(out[F] == SENT) and np.all(q[F] == SENT), "written outside the F rows"
                    assert m[F] == SENT and r[F] == SENT and n[F] == -7, "written outside the F rows"
                    assert not np.isnan(out).any() and not np.isnan(q).any() and not n[:F].any() and np.abs(out[:F, :C]).max() < 8.0
                    out, q, m, r = out[:F, :C], q[:F], m[:F], r[:F]
                    # frames outside every segment, or alone in their own: the row and its quaternions bit for bit, zeros beside them
                    assert np.array_equal(out[alone], src[alone]) and np.array_equal(q[alone], quat[alone]), (H, D, kind)
                    assert not m[alone].any() and not r[alone].any()
                    qc = q.astype(np.float64)
                    qc[alone] = rref.canonical(qc[alone])
                    worst["dst"], worst["quat"] = max(worst["dst"], ref.within(out, want)), max(worst["quat"], ref.within(qc, rref.canonical(want_q)))
                    worst["moved"], worst["rot_moved"] = max(worst["moved"], ref.within(m, want_m)), max(worst["rot_moved"], ref.within(r, want_r))
                    # unit quaternions of canonical sign, rigid skeletons, and dst is what the stored quaternions lay from dst's roots
                    worst["unit"] = max(worst["unit"], np.abs(np.linalg.norm(q.astype(np.float64), axis=2) - 1.0).max())
                    assert _canonical_sign(q[~alone]), (H, D, kind)
                    worst["length"] = max(worst["length"], np.abs(bref.bone_lengths(out[~alone], bones) - L).max() if (~alone).any() else 0.0)
                    worst["fk"] = max(worst["fk"], np.abs(_fk(out, q, bones, body) - out)[~alone].max() if (~alone).any() else 0.0)
                    # the roots: the column form's bits
                    plain = torch.full((F, C), SENT, dtype=torch.float32, device=dev)
                    hip.call("smooth_frames", _d(dev, src), C, F, C, _d(dev, seg), _d(dev, w), H, D, plain, C, None)
                    assert torch.equal(dst[:F, cols], plain[:, cols]), (H, D, kind)
                    # two launches, the same bits; without the three optional outputs the same dst and quat_out, those buffers untouched
                    again = _raw(dev, src, quat, seg, w, D, J, bones, body, pad_s, pad_d)
                    assert all(torch.equal(a, b) for a, b in zip((dst, qo, mv, rm, fb), again)), (H, D, kind)
                    dst3, qo3, mv3, rm3, fb3 = _raw(dev, src, quat, seg, w, D, J, bones, body, pad_s, pad_d, moved=False, rot_moved=False,
                                                    fallback=False)
                    assert torch.equal(dst, dst3) and torch.equal(qo, qo3), (H, D, kind)
                    assert bool((mv3 == SENT).all()) and bool((rm3 == SENT).all()) and bool((fb3 == -7).all())
                    for keep in ("moved", "rot_moved", "fallback"):          # (each alone, too)
                        one = _raw(dev, src, quat, seg, w, D, J, bones, body, pad_s, pad_d, **{k: k == keep for k in ("moved", "rot_moved", "fallback")})
                        assert torch.equal(dst, one[0]) and torch.equal(qo, one[1]), (H, D, kind, keep)
                        assert torch.equal({"moved": mv, "rot_moved": rm, "fallback": fb}[keep], one[2 + ("moved", "rot_moved", "fallback").index(keep)])
                    # the sign of an input quaternion does not matter (a copied row copies it)
                    dst4, qo4, mv4, rm4, fb4 = _raw(dev, src, quat * flip, seg, w, D, J, bones, body, pad_s, pad_d)
                    assert torch.equal(dst, dst4) and torch.equal(mv, mv4) and torch.equal(rm, rm4) and torch.equal(fb, fb4), (H, D, kind)
                    q4 = qo4.cpu().numpy()[:F]
                    assert np.array_equal(q4[~alone], q[~alone]) and np.array_equal(q4[alone], (quat * flip)[alone]), (H, D, kind)
                    # what lies outside a segment does not reach into it
                    if inside.any() and not inside.all():
                        src5, quat5 = src.copy(), quat.copy()
                        src5[~inside], quat5[~inside] = other[0][~inside], other[1][~inside]
                        got = _raw(dev, src5, quat5, seg, w, D, J, bones, body, pad_s, pad_d)
                        idx = torch.as_tensor(np.flatnonzero(inside)).to(dev)
                        assert all(torch.equal(a[idx], b[idx]) for a, b in zip((dst, qo, mv, rm, fb), got)), (H, D, kind)
    least = min(gaps) if gaps else float("inf")
    print("%s F %d: worst error / bound %.3f (dst) %.3f (quat) %.3f (moved) %.3f (rot_moved); | |bone| - L | %.3e m, | |q| - 1 | %.3e, "
          "FK of quat_out against dst %.3e m; least gap / sum |c| %.3f, largest sum |c| %.3f over %d launches" % (
              tree, F, worst["dst"], worst["quat"], worst["moved"], worst["rot_moved"], worst["length"], worst["unit"], worst["fk"], least,
              max(sums) if sums else 0.0, case))
    assert least >= 1e-3, "the restatement's eigenvector is well conditioned on these rows"
    assert worst["dst"] <= 1.0 and worst["quat"] <= 1.0 and worst["moved"] <= 1.0 and worst["rot_moved"] <= 1.0
    assert worst["length"] <= RIGID and worst["unit"] <= UNIT and worst["fk"] <= JOINT


def steady_rows(rng, F, tree, omega):
    """Rows whose roots stand still and whose bones turn about a fixed axis each at ``omega`` radians a frame (0: a constant sequence).
    -> (src, quat float32 with random signs, the exact positions and canonical quaternions float64, body)."""
    J, bones = TREES[tree]
    NB = len(bones)
    body = _body(rng, NB)
    base = rsref.jittery_rotations(rng, 1, NB)[0]
    axes = rng.normal(size=(NB, 3))
    rot = np.stack([np.stack([rsref.axis_angle(axes[b], omega * f) @ base[b] for b in range(NB)]) for f in range(F)])
    roots = np.tile(rng.normal(0.0, 0.7, (1, J, 3)), (F, 1, 1))
    return rsref.rows_of(rng, rot, bones, body, J, roots=roots) + (body,)


@pytest.mark.parametrize("tree", ["upper", "lower"])
@pytest.mark.parametrize("omega", [0.0, 0.02])
def test_constant_rotations_and_constant_velocity_come_back(dev, tree, omega):
    """Through ops, one segment of 70 frames.  omega = 0: every frame comes back.  omega = 0.02 rad a frame: every frame whose taps are
    symmetric (H <= f < F - H, symmetric tables) comes back, for every order -- the odd terms cancel and sum_k c_k cos(k omega) > 0
    (asserted in tests/test_rot_smooth_cpu.py).  Against the EXACT rotations and positions, within the bound: the float rounding of the
    input quaternions (2^-25 a component) passes through with a gain of at most sum |c_k|."""
    from mmego_amd import ops
    J, bones = TREES[tree]
    F, NB = 70, len(bones)
    rng = np.random.default_rng(int(1000 * omega) + J)
    src, quat, pos64, q64, body = steady_rows(rng, F, tree, omega)
    assert np.abs(src).max() < 8.0
    seg = np.zeros(F, np.int32)
    worst_p = worst_q = 0.0
    for H in HS:
        frames = np.arange(F) if omega == 0.0 else np.arange(H, F - H)
        assert len(frames) >= 8
        for D in DS:
            for kind in ("box", "gauss"):
                dst = torch.full((F, 3 * J), SENT, dtype=torch.float32, device=dev)
                qo = torch.full((F, NB, 4), SENT, dtype=torch.float32, device=dev)
                fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
                ops.smooth_rot(_d(dev, src), _d(dev, quat), seg, sref.weights(H, kind), D, np.asarray(bones), body, dst, qo, None, None, fb)
                assert not fb.cpu().numpy().any()
                worst_p = max(worst_p, ref.within(dst.cpu().numpy()[frames], pos64[frames]))
                worst_q = max(worst_q, ref.within(qo.cpu().numpy()[frames], q64[frames]))
    print("%s omega %g: worst error / bound %.3f (dst) %.3f (quat) against the exact sequence" % (tree, omega, worst_p, worst_q))
    assert worst_p <= 1.0 and worst_q <= 1.0


def test_a_half_turn_between_two_frames_keeps_each_frames_own_rotation(dev):
    """Two frames of one segment under order 0 and the box table of H = 1: both weigh their two valid taps 1 / 2 each.  The neck bone
    (bone 0 of the upper walk) is the identity in frame 0 and a half turn about z in frame 1: S = diag(0, 0, 1), the 4 x 4 matrix
    diag(1, -1, -1, 1), its two largest eigenvalues equal (the restatement's gap is 0 up to the rounding of its least-squares
    coefficients, asserted first): each frame keeps its own rotation and counts one fallback; the other bones, constant, come back."""
    from mmego_amd import dense, ops
    J, bones = TREES["upper"]
    rng = np.random.default_rng(11)
    body = _body(rng, 14)
    rot = np.tile(rsref.jittery_rotations(rng, 1, 14), (2, 1, 1, 1))
    rot[0, 0], rot[1, 0] = np.eye(3), np.diag([-1.0, -1.0, 1.0])
    src, quat, _, _ = rsref.rows_of(rng, rot, bones, body, J, signs=False)
    assert quat[0, 0].tolist() == [1, 0, 0, 0] and quat[1, 0].tolist() == [0, 0, 0, 1]
    seg, w = np.array([4, 4], np.int32), dense.smooth_weights(1, "box")
    gaps = []
    want, want_q, want_m, want_r, want_fb = rsref.smooth_rot(src, quat, seg, w, 0, bones, body, min_gap=gaps)
    assert len(gaps) == 2 and max(gaps) <= 1e-15 and want_fb.tolist() == [1, 1]
    dst = torch.full((2, 45), SENT, dtype=torch.float32, device=dev)
    qo = torch.full((2, 14, 4), SENT, dtype=torch.float32, device=dev)
    mv, rm = (torch.full((2,), SENT, dtype=torch.float32, device=dev) for _ in range(2))
    fb = torch.full((2,), -7, dtype=torch.int32, device=dev)
    ops.smooth_rot(_d(dev, src), _d(dev, quat), seg, w, 0, np.asarray(bones), body, dst, qo, mv, rm, fb)
    q = qo.cpu().numpy()
    assert fb.cpu().numpy().tolist() == [1, 1]
    assert q[0, 0].tolist() == [1, 0, 0, 0] and q[1, 0].tolist() == [0, 0, 0, 1]
    assert ref.within(dst.cpu().numpy(), want) <= 1.0 and ref.within(q, want_q) <= 1.0
    assert ref.within(mv.cpu().numpy(), want_m) <= 1.0 and ref.within(rm.cpu().numpy(), want_r) <= 1.0
    assert np.abs(bref.bone_lengths(dst.cpu().numpy(), bones) - np.linalg.norm(body.astype(np.float64), axis=1)).max() <= RIGID
    # at order 2 the degree falls to 1, the line through two taps is evaluated at one of them: nothing is averaged, no fallback
    ops.smooth_rot(_d(dev, src), _d(dev, quat), seg, w, 2, np.asarray(bones), body, dst, qo, mv, rm, fb)
    assert not fb.cpu().numpy().any() and ref.within(qo.cpu().numpy(), rref.canonical(quat)) <= 1.0
    # with the second frame in no segment nothing is filtered: rows and quaternions bit for bit
    ops.smooth_rot(_d(dev, src), _d(dev, quat), np.array([4, -1], np.int32), w, 0, np.asarray(bones), body, dst, qo, mv, rm, fb)
    assert np.array_equal(dst.cpu().numpy(), src) and np.array_equal(qo.cpu().numpy(), quat)
    assert not mv.cpu().numpy().any() and not rm.cpu().numpy().any() and not fb.cpu().numpy().any()


def test_refusals_leave_the_outputs_alone(dev):
    from mmego_amd import dense, hip, ops
    J, bones = TREES["upper"]
    rng = np.random.default_rng(5)
    body = _body(rng, 14)
    F = 9
    src_h, quat_h, _, _ = rsref.rows_of(rng, rsref.jittery_rotations(rng, F, 14), bones, body, J)
    src, quat = _d(dev, src_h), _d(dev, quat_h)
    seg = np.zeros(F, np.int32)
    w = dense.smooth_weights(2, "gauss")
    dst = torch.full((F, 45), SENT, dtype=torch.float32, device=dev)
    qo = torch.full((F, 14, 4), SENT, dtype=torch.float32, device=dev)
    mv, rm = (torch.full((F,), SENT, dtype=torch.float32, device=dev) for _ in range(2))
    fb = torch.full((F,), -7, dtype=torch.int32, device=dev)
    walk = np.asarray(bones)
    twice = walk.copy()
    twice[5] = [3, 4]                                                  # joint 3 is bone 0's child already
    late = walk.copy()
    late[[0, 1]] = late[[1, 0]]                                        # (2, 3) ahead of (3, 14): the parent comes after its child
    zero = body.copy()
    zero[4] = 0.0
    odd = torch.full((F * 14 * 4 + 4,), SENT, dtype=torch.float32, device=dev)
    for what, call in (("a child listed twice", lambda: ops.smooth_rot(src, quat, seg, w, 2, twice, body, dst, qo, mv, rm, fb)),
                       ("a parent after its child", lambda: ops.smooth_rot(src, quat, seg, w, 2, late, body, dst, qo, mv, rm, fb)),
                       ("a zero rest bone", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, zero, dst, qo, mv, rm, fb)),
                       ("one rest bone too few", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, body[:-1], dst, qo, mv, rm, fb)),
                       ("body of lengths", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, body[:, 0], dst, qo, mv, rm, fb)),
                       ("rows that are no 3-vectors", lambda: ops.smooth_rot(src[:, :44], quat, seg, w, 2, walk, body, dst, qo, mv, rm, fb)),
                       ("dst is src", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, body, src, qo, mv, rm, fb)),
                       ("quat_out is quat", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, body, dst, quat, mv, rm, fb)),
                       ("a short quat", lambda: ops.smooth_rot(src, quat[:-1], seg, w, 2, walk, body, dst, qo, mv, rm, fb)),
                       ("quaternions of three", lambda: ops.smooth_rot(src, quat[:, :, :3].contiguous(), seg, w, 2, walk, body, dst, qo, mv, rm, fb)),
                       ("a double quat", lambda: ops.smooth_rot(src, quat.double(), seg, w, 2, walk, body, dst, qo, mv, rm, fb)),
                       ("a misaligned quat_out", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, body, dst, odd[1:-3].view(F, 14, 4), mv, rm, fb)),
                       ("an even weight length", lambda: ops.smooth_rot(src, quat, seg, w[:-1], 2, walk, body, dst, qo, mv, rm, fb)),
                       ("order 3", lambda: ops.smooth_rot(src, quat, seg, w, 3, walk, body, dst, qo, mv, rm, fb)),
                       ("a short seg", lambda: ops.smooth_rot(src, quat, seg[:-1], w, 2, walk, body, dst, qo, mv, rm, fb)),
                       ("a short rot_moved", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, body, dst, qo, mv, rm[:-1], fb)),
                       ("a float fallback", lambda: ops.smooth_rot(src, quat, seg, w, 2, walk, body, dst, qo, mv, rm, mv))):
        with pytest.raises((ValueError, IndexError, TypeError)):
            call()
        torch.cuda.synchronize()
        assert bool((dst == SENT).all()) and bool((qo == SENT).all()) and bool((odd == SENT).all()), what
        assert bool((mv == SENT).all()) and bool((rm == SENT).all()) and bool((fb == -7).all()), what
        assert torch.equal(src, _d(dev, src_h)) and torch.equal(quat, _d(dev, quat_h)), what
    segd, wd, bd, yd = _d(dev, seg), _d(dev, w), _d(dev, walk.astype(np.int32)), _d(dev, body)
    good = dict(src=src, lds=45, F=F, J=J, quat=quat, NB=14, seg=segd, w=wd, H=2, D=2, bones=bd, body=yd, dst=dst, ldd=45, quat_out=qo,
                moved=mv, rot_moved=rm, fallback=fb)
    for change in (dict(src=None), dict(quat=None), dict(seg=None), dict(w=None), dict(bones=None), dict(body=None), dict(dst=None),
                   dict(quat_out=None), dict(F=0), dict(F=-1), dict(F=1 << 31), dict(J=1), dict(J=22, lds=66, ldd=66), dict(NB=0), dict(NB=15),
                   dict(lds=44), dict(ldd=44), dict(H=0), dict(H=32), dict(D=-1), dict(D=3), dict(quat=odd[1:]), dict(quat_out=odd[1:]),
                   dict(dst=src), dict(quat_out=quat)):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("smooth_rot", *[a[k] for k in good])
    torch.cuda.synchronize()
    assert bool((dst == SENT).all()) and bool((qo == SENT).all()) and bool((odd == SENT).all())
    assert bool((mv == SENT).all()) and bool((rm == SENT).all()) and bool((fb == -7).all())
    assert torch.equal(src, _d(dev, src_h)) and torch.equal(quat, _d(dev, quat_h))
    ops.smooth_rot(src, quat, seg, w, 2, walk, body, dst, qo, mv, rm, fb)            # (and the good call goes through)
    assert not bool((dst == SENT).any()) and not bool((qo == SENT).any()) and not bool((fb == -7).any())
