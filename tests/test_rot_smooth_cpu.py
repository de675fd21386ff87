"""CPU: --rot_smooth / --rot_smooth_order / --rot_smooth_taper on the command line (defaults, refusals, what reaches ConfigDemo), the
declaration and the export of mmego_smooth_rot, the checks of dense_infer's rot_smooth argument that need no device, the host figure
dense.rot_jitter_deg, and properties of the restatement of tests/rot_smooth_ref.py itself: at order 0 it is rot_blend_ref's chordal mean,
a constant sequence and a constant angular velocity come back."""
import ctypes

import numpy as np
import pytest

import main as cli
import rot_blend_ref as rref
import rot_smooth_ref as rsref
import smooth_ref as sref


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_rot_smooth_reaches_the_config_and_is_off_by_default():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "upper_variant", "metrics", "smooth", "rot_smooth",
             "floor")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    assert ConfigDemo.rot_smooth is None
    rot = ["--infer", "--dense", "--blend_space", "rot"]
    try:
        for argv, want in ((rot + ["--rot_smooth", "4"], (4, 2, "gauss")),
                           (rot + ["--rot_smooth", "1", "--rot_smooth_order", "0"], (1, 0, "gauss")),
                           (rot + ["--rot_smooth", "31", "--rot_smooth_taper", "box", "--rot_smooth_order", "1"], (31, 1, "box")),
                           (rot + ["--rot_smooth", "2", "--floor", "measure", "--save_pred", "x.npz"], (2, 2, "gauss")),
                           (rot, None), (["--infer", "--dense"], None), (["--infer"], None)):
            args = p.parse_args(argv)
            cli.check_dense(p, args)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert ConfigDemo.rot_smooth == want and ConfigDemo.smooth is None, argv
    finally:
        for c, k, v in keep:                         # (what the class itself held; what it inherits comes back by deleting the override)
            if v is not missing:
                setattr(c, k, v)
            elif k in c.__dict__:
                delattr(c, k)
    args = p.parse_args(rot)
    assert args.rot_smooth is None and args.rot_smooth_order is None and args.rot_smooth_taper is None
    assert "--rot_smooth H" in cli.__doc__


@pytest.mark.parametrize("flag", [["--rot_smooth", "4"], ["--rot_smooth_order", "1"], ["--rot_smooth_taper", "box"]])
def test_the_rot_smooth_flags_need_dense(capsys, monkeypatch, flag):
    for head in (["--infer"], ["--train", "--network", "Upper_Net"], []):
        err = _refused(head + flag, capsys, monkeypatch)
        assert "%s belongs to --infer --dense" % flag[0] in err, head


@pytest.mark.parametrize("space", [[], ["--blend_space", "joints"], ["--blend_space", "bones"]])
def test_rot_smooth_needs_blend_space_rot(capsys, monkeypatch, space):
    err = _refused(["--infer", "--dense"] + space + ["--rot_smooth", "3"], capsys, monkeypatch)
    assert "--rot_smooth belongs to --dense --blend_space rot" in err


@pytest.mark.parametrize("flag", [["--rot_smooth_order", "1"], ["--rot_smooth_taper", "box"]])
def test_order_and_taper_need_rot_smooth(capsys, monkeypatch, flag):
    err = _refused(["--infer", "--dense", "--blend_space", "rot"] + flag, capsys, monkeypatch)
    assert "%s belongs to --rot_smooth H" % flag[0] in err


@pytest.mark.parametrize("H", ["0", "32", "-3"])
def test_a_half_width_outside_1_to_31_is_refused(capsys, monkeypatch, H):
    err = _refused(["--infer", "--dense", "--blend_space", "rot", "--rot_smooth", H], capsys, monkeypatch)
    assert "--rot_smooth is the filter's half-width in frames" in err


def test_other_values_and_the_old_refusals(capsys, monkeypatch):
    rot = ["--infer", "--dense", "--blend_space", "rot"]
    assert "invalid choice" in _refused(rot + ["--rot_smooth", "4", "--rot_smooth_order", "3"], capsys, monkeypatch)
    assert "invalid choice" in _refused(rot + ["--rot_smooth", "4", "--rot_smooth_taper", "hann"], capsys, monkeypatch)
    assert "invalid int value" in _refused(rot + ["--rot_smooth", "2.5"], capsys, monkeypatch)
    # --smooth stays refused under rot, with or without the new flag, and now points at it; so does --floor clamp
    for more in ([], ["--rot_smooth", "3"]):
        err = " ".join(_refused(rot + ["--smooth", "3"] + more, capsys, monkeypatch).split())
        assert "--smooth does not go with --blend_space rot" in err and "would not be filtered with the positions" in err
        assert "--rot_smooth H" in err
    assert "--floor clamp does not go with --blend_space rot" in _refused(rot + ["--rot_smooth", "3", "--floor", "clamp"], capsys, monkeypatch)


def test_the_entry_point_is_declared_as_ops_calls_it_and_exported():
    from mmego_amd import build, hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_smooth_rot"]] == ["stream", "src", "lds", "F", "J", "quat", "NB", "seg", "w", "H", "D", "bones",
                                                          "body", "dst", "ldd", "quat_out", "moved", "rot_moved", "fallback"]
    assert callable(ops.smooth_rot)
    assert hasattr(ctypes.CDLL(build.build_library()), "mmego_smooth_rot")


def test_the_rot_smooth_argument_is_checked_before_anything_runs():
    """dense_infer checks its arguments before it builds the plan: a bad call never reads ``dataset`` (None here)."""
    from mmego_amd import dense
    assert dense._check_smooth(None, "rot_smooth") is None
    assert dense._check_smooth((np.int64(3), 2, "box"), "rot_smooth") == (3, 2, "box")
    call = lambda **kw: dense.dense_infer(None, None, None, None, None, 3, **kw)
    for bad in ((3, 2), (0, 2, "box"), (32, 2, "box"), (3, 3, "box"), (3, -1, "box"), (3, 1.0, "box"), (3, 2, "hann"), "gauss", 3):
        with pytest.raises(ValueError, match="^rot_smooth: "):
            call(blend_space="rot", rot_smooth=bad)
    for space in (None, "joints", "bones"):
        with pytest.raises(ValueError, match="rot_smooth: .*only blend_space=\"rot\" keeps"):
            call(blend_space=space, rot_smooth=(3, 2, "gauss"))
    with pytest.raises(ValueError, match="would not be filtered"):
        call(blend_space="rot", smooth=(3, 2, "gauss"), rot_smooth=(3, 2, "gauss"))
    with pytest.raises(ValueError, match="would not be filtered.*rot_smooth"):
        call(blend_space="rot", smooth=(3, 2, "gauss"))
    with pytest.raises(ValueError, match="floor: the clamp moves joint positions"):
        call(blend_space="rot", rot_smooth=(3, 2, "gauss"), floor=("clamp", 6, 0))
    with pytest.raises(ValueError, match="^smooth: "):             # (the old keyword keeps its own name in its refusals)
        call(smooth=(0, 2, "box"))


def test_cpu_tensors_are_refused_before_any_launch(monkeypatch):
    import torch
    from mmego_amd import dense, hip, ops, skeleton

    def no_launch(*a, **k):
        raise AssertionError("a launch was attempted")
    monkeypatch.setattr(hip, "call", no_launch)
    rng = np.random.default_rng(0)
    body = rng.normal(0, 0.3, (14, 3)).astype(np.float32)
    src, quat, _, _ = rsref.rows_of(rng, rsref.jittery_rotations(rng, 6, 14), rref.UPPER_WALK, body, 15)
    src, quat = torch.from_numpy(src), torch.from_numpy(quat)
    dst, qo = torch.full((6, 45), -1.0), torch.full((6, 14, 4), -1.0)
    with pytest.raises(TypeError):
        ops.smooth_rot(src, quat, np.zeros(6, np.int32), dense.smooth_weights(2, "gauss"), 2, skeleton.WALK_UPPER, body, dst, qo)
    assert bool((dst == -1.0).all()) and bool((qo == -1.0).all())


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def test_rot_jitter_by_hand():
    """One bone turning about z by the angles 0, 0.1, 0.3, 0.3, 0.3 (radians): the turn per frame is 0.1, 0.2, 0, 0, so the change of
    the turn is 0.1, 0.2, 0 at the three inner frames.  A recording's edge, an uncovered neighbour and a quaternion's sign take no part."""
    from mmego_amd import dense
    ang = np.array([0.0, 0.1, 0.3, 0.3, 0.3])
    q = np.zeros((5, 1, 4))
    q[:, 0, 0], q[:, 0, 3] = np.cos(ang / 2), np.sin(ang / 2)
    q[2] *= -1.0
    rec, cov = np.zeros(5, np.int64), np.ones(5, np.int32)
    assert np.isclose(dense.rot_jitter_deg(q, rec, cov), np.degrees((0.1 + 0.2 + 0.0) / 3), rtol=0, atol=1e-12)
    assert np.isclose(dense.rot_jitter_deg(q, np.array([0, 0, 0, 1, 1]), cov), np.degrees(0.1), rtol=0, atol=1e-12)
    assert np.isclose(dense.rot_jitter_deg(q, rec, np.array([1, 1, 1, 1, 0])), np.degrees(0.15), rtol=0, atol=1e-12)
    nan = q.copy()
    nan[4] = np.nan                                                      # (an uncovered frame's NaN quaternion never enters)
    assert np.isclose(dense.rot_jitter_deg(nan, rec, np.array([1, 1, 1, 1, 0])), np.degrees(0.15), rtol=0, atol=1e-12)
    assert dense.rot_jitter_deg(q, np.array([0, 0, 1, 1, 2]), cov) is None and dense.rot_jitter_deg(q[:2], rec[:2], cov[:2]) is None


def test_order_0_is_the_chordal_mean_of_rot_blend_ref():
    """Order 0 with positive weights: c_k = w_k / sum w, so the filtered rotation is mmego_blend_rot's weighted chordal mean of the same
    rotations (rot_blend_ref takes it from an SVD, this restatement from eigh), and the roots are the weighted means."""
    rng = np.random.default_rng(5)
    F, J, bones, H = 9, 15, rref.UPPER_WALK, 3
    body = rng.normal(0, 0.3, (14, 3)).astype(np.float32)
    src, quat, _, _ = rsref.rows_of(rng, rsref.jittery_rotations(rng, F, 14), bones, body, J)
    seg = np.zeros(F, np.int32)
    w = rng.uniform(0.5, 2.0, 2 * H + 1).astype(np.float32)
    dst, qo, moved, rmoved, fb = rsref.smooth_rot(src, quat, seg, w, 0, bones, body)
    # the same frames as a cover: frame f is served by the rows f + k of its valid taps with the weights w_k; Rh = I and q = the matrices
    off, row, cw = [0], [], []
    for f in range(F):
        taps = sref.valid_taps(seg, f, H)
        row += [f + k for k in taps]
        cw += [w[k + H] for k in taps]
        off.append(len(row))
    A = rsref.matrices(quat).reshape(F, 14, 9)
    Rh = np.tile(np.eye(3).reshape(9), (F, 1))
    want, wq, _, _, wfb = rref.blend_rot(src, A, Rh, np.asarray(off, np.int64), np.asarray(row, np.int32), np.asarray(cw, np.float32), bones,
                                         tuple(range(14)), body)
    assert not fb.any() and not wfb.any()
    assert np.abs(dst - want).max() <= 1e-13 and np.abs(qo - wq).max() <= 1e-13 and moved.min() > 1e-3 and rmoved.min() > 1e-2


@pytest.mark.parametrize("D", [0, 1, 2])
def test_constant_rotations_and_constant_velocity_come_back(D):
    """A constant sequence comes back on every frame (the coefficients sum to 1).  A rotation about a fixed axis at omega radians a
    frame comes back on every frame whose valid taps are symmetric: S = sum_k c_k R(k omega) A_0, the odd terms cancel (c_-k = c_k), and
    what is left is (sum_k c_k cos(k omega)) on the plane of the rotation, positive for omega = 0.02 at H <= 31 (asserted)."""
    rng = np.random.default_rng(7 + D)
    J, bones, omega = 8, rref.LOWER_WALK, 0.02
    body = rng.normal(0, 0.3, (6, 3))
    for H, F in ((1, 9), (3, 12), (31, 70)):
        w = sref.weights(H, "gauss") if H != 3 else rng.uniform(0.5, 2.0, 2 * H + 1).astype(np.float32)
        w = np.maximum(w, w[::-1])                                       # (symmetric weights: c_-k = c_k)
        seg = np.zeros(F, np.int32)
        base = rsref.jittery_rotations(rng, 1, 6)[0]
        axes = rng.normal(size=(6, 3))
        still = np.tile(base[None], (F, 1, 1, 1))
        turning = np.stack([np.stack([rsref.axis_angle(axes[b], omega * f) @ base[b] for b in range(6)]) for f in range(F)])
        roots = np.tile(rng.normal(0, 0.7, (1, J, 3)), (F, 1, 1))
        for rot, frames in ((still, range(F)), (turning, range(H, F - H))):
            pos = roots.copy()
            quat = np.zeros((F, 6, 4))
            for f in range(F):
                for b, (c, p) in enumerate(bones):
                    pos[f, c] = pos[f, p] + rot[f, b] @ body[b]
                    quat[f, b] = rref.quaternion(rot[f, b])
            dst, qo, moved, rmoved, fb = rsref.smooth_rot(pos.reshape(F, 24), quat, seg, w, D, bones, body)
            frames = list(frames)
            assert len(frames) >= 2 and not fb.any()
            c = sref.coefficients(w, list(range(-H, H + 1)), D)
            assert (c * np.cos(np.arange(-H, H + 1) * omega)).sum() > 0.5
            assert np.abs(qo[frames] - quat[frames]).max() <= 1e-13 and np.abs(dst[frames] - pos.reshape(F, 24)[frames]).max() <= 1e-13
            assert moved[frames].max() <= 1e-13 and rmoved[frames].max() <= 1e-7       # (an angle near 0 from atan2(|v|, .): sqrt of rounding)


def test_a_half_turn_between_two_frames_has_no_mean():
    """Two frames of one segment, box weights, H = 1, order 0: two valid taps with c = (1/2, 1/2).  (At order 1 or 2 the degree falls
    to 1 and the line through two taps is evaluated at one of them: c = (1, 0), nothing is averaged -- asserted.)  The bone is the
    identity in frame 0 and a half turn about z in frame 1: S = diag(0, 0, 1), the 4 x 4 matrix diag(1, -1, -1, 1) -- its two largest
    eigenvalues are equal, each frame keeps its own rotation and counts one fallback."""
    body = np.array([[0.25, 0.0, 0.0]])
    quat = np.array([[[1.0, 0, 0, 0]], [[0, 0, 0, 1.0]]])
    src = np.array([[0.5, 0.25, -0.75, 0.75, 0.25, -0.75], [1.0, 0.25, -0.75, 0.75, 0.25, -0.75]])
    gaps = []
    dst, qo, moved, rmoved, fb = rsref.smooth_rot(src, quat, np.zeros(2, np.int32), np.ones(3, np.float32), 0, ((1, 0),), body, min_gap=gaps)
    assert np.allclose(sref.coefficients(np.ones(3), [0, 1], 0), [0.5, 0.5], rtol=0, atol=1e-15)
    assert np.allclose(sref.coefficients(np.ones(3), [0, 1], 2), [1.0, 0.0], rtol=0, atol=1e-15)
    # (0 up to the rounding of the least-squares coefficients, 1/2 to an ulp; the fallback's threshold is 1e-9)
    assert len(gaps) == 2 and max(gaps) <= 1e-15 and fb.tolist() == [1, 1]
    assert qo[0, 0].tolist() == [1, 0, 0, 0] and qo[1, 0].tolist() == [0, 0, 0, 1] and rmoved.tolist() == [0.0, 0.0]
    assert np.allclose(dst, [[0.75, 0.25, -0.75, 1.0, 0.25, -0.75], [0.75, 0.25, -0.75, 0.5, 0.25, -0.75]], rtol=0, atol=1e-15)
