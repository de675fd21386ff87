"""CPU: --blend_space rot on the command line, the rotation tables of mmego_amd/skeleton.py, the declaration of mmego_blend_rot, the host
checks ops.blend_rot makes before it launches, and the restatement of tests/rot_blend_ref.py on cases worked out by hand."""
import numpy as np
import pytest

import main as cli
import rot_blend_ref as rref


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_blend_space_rot_reaches_the_config():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "upper_variant", "metrics", "smooth")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    try:
        for argv, want in ((["--infer", "--dense", "--blend_space", "rot"], "rot"),
                           (["--infer", "--dense", "--stride", "3", "--blend_space", "rot", "--save_pred", "x.npz"], "rot"),
                           (["--infer", "--dense"], None)):
            args = p.parse_args(argv)
            cli.check_dense(p, args)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert ConfigDemo.blend_space == want, argv
    finally:
        for c, k, v in keep:                         # (what the class itself held; what it inherits comes back by deleting the override)
            if v is not missing:
                setattr(c, k, v)
            elif k in c.__dict__:
                delattr(c, k)
    from mmego_amd import dense
    assert dense.BLEND_SPACES == ("joints", "bones", "rot")


def test_blend_space_rot_needs_dense(capsys, monkeypatch):
    for head in (["--infer"], ["--train", "--network", "Upper_Net"], []):
        err = _refused(head + ["--blend_space", "rot"], capsys, monkeypatch)
        assert "--blend_space belongs to --infer --dense" in err, head


def test_blend_space_rot_is_refused_with_smooth(capsys, monkeypatch):
    err = _refused(["--infer", "--dense", "--blend_space", "rot", "--smooth", "3"], capsys, monkeypatch)
    assert "--smooth does not go with --blend_space rot" in err and "would not be filtered with the positions" in " ".join(err.split())


def test_the_entry_point_is_declared_as_ops_calls_it():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_blend_rot"]] == ["stream", "src", "nrows", "J", "q", "NQ", "Rh", "cov_off", "cov_row", "cov_w", "F",
                                                         "bones", "rot_idx", "body", "NB", "dst", "ldd", "quat", "spread", "rot_spread",
                                                         "fallback"]
    assert callable(ops.blend_rot)


def test_rotation_tables_agree_with_the_fk_plans():
    from mmego_amd import skeleton
    from oracle import skeleton as osk
    up, lo = osk.upper_fk_plan(), osk.lower_fk_plan()
    # bone k of the walk: the oracle's (parent slot, child slot); Upper_Net turns it by q[child slot], Lower_Net by q[rot row]
    assert skeleton.WALK_UPPER.tolist() == [[c, p] for p, c, _ in up] and [i for _, _, i in up] == list(skeleton.WALK_UPPER_ROWS)
    assert skeleton.ROT_UPPER == [c for _, c, _ in up] == [3, 2, 1, 4, 8, 5, 6, 7, 9, 10, 11, 0, 12, 13]
    assert skeleton.WALK_LOWER.tolist() == [[c, p] for p, c, _, _ in lo] and [i for _, _, _, i in lo] == list(skeleton.WALK_LOWER_ROWS)
    assert skeleton.ROT_LOWER == [r for _, _, r, _ in lo] == [0, 1, 2, 3, 4, 5]
    assert tuple(skeleton.LOWER_ROT_MAP) == osk.LOWER_ROT_MAP
    assert list(rref.ROT_UPPER) == skeleton.ROT_UPPER and list(rref.ROT_LOWER) == skeleton.ROT_LOWER


def test_cpu_tensors_are_refused_before_any_launch(monkeypatch):
    import torch
    from mmego_amd import hip, ops, skeleton

    def no_launch(*a, **k):
        raise AssertionError("a launch was attempted")
    monkeypatch.setattr(hip, "call", no_launch)
    rng = np.random.default_rng(0)
    body = rng.normal(0, 0.3, (14, 3)).astype(np.float32)
    src, q, Rh = (torch.from_numpy(a) for a in rref.rigid_rows(rng, 6, 15, rref.UPPER_WALK, rref.ROT_UPPER, 14, body))
    cover = (np.array([0, 2, 3], np.int64), np.array([0, 1, 5], np.int32), np.array([1, 2, 1], np.float32))
    dst, quat = torch.full((2, 45), -1.0), torch.full((2, 14, 4), -1.0)
    with pytest.raises(TypeError, match="fp32 device tensor"):
        ops.blend_rot(src, q, Rh, cover, skeleton.WALK_UPPER, skeleton.ROT_UPPER, body, dst, quat)
    with pytest.raises(TypeError):
        ops.blend_rot(src.double(), q, Rh, cover, skeleton.WALK_UPPER, skeleton.ROT_UPPER, body, dst, quat)
    assert bool((dst == -1.0).all()) and bool((quat == -1.0).all())


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def _one_bone(mats, weights, Rh=None, src=None):
    """One frame over len(mats) rows of a two-joint skeleton whose single bone (1, 0) has the world rotations ``mats``."""
    n = len(mats)
    Rh = np.tile(np.eye(3), (n, 1, 1)) if Rh is None else np.asarray(Rh)
    q = np.stack([h @ m for h, m in zip(Rh, mats)]).reshape(n, 1, 9)
    body = np.array([[0.5, 0.0, 0.0]])
    if src is None:
        src = np.stack([np.concatenate([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0] + m @ body[0]]) for m in mats])
    off = np.array([0, n], np.int64)
    return rref.blend_rot(src, q, Rh.reshape(n, 9), off, np.arange(n, dtype=np.int32), np.asarray(weights, np.float32), ((1, 0),), (0,), body)


def test_the_restatement_on_cases_worked_by_hand():
    a = 0.7
    # +a and -a about z at equal weight: the identity; the bone lies along x from the common root
    dst, quat, spr, rspr, fb = _one_bone([_rz(a), _rz(-a)], (2, 2))
    assert np.allclose(quat[0, 0], [1, 0, 0, 0], rtol=0, atol=1e-15) and fb[0] == 0
    assert np.allclose(dst[0], [1, 2, 3, 1.5, 2, 3], rtol=0, atol=1e-15)
    assert np.isclose(rspr[0], a, rtol=1e-14)                       # both windows lie a radians from the mean
    # the same behind a head rotation: Rh^T q is the world rotation again
    H = _rz(1.1) @ np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])
    assert np.allclose(_one_bone([_rz(a), _rz(-a)], (2, 2), Rh=[H, H.T])[1][0, 0], [1, 0, 0, 0], rtol=0, atol=1e-15)
    # weights 3 : 1 at angles 0 and a: S = 3 I + Rz(a), the mean turns by atan2(sin a, 3 + cos a)
    dst, quat, _, _, fb = _one_bone([np.eye(3), _rz(a)], (3, 1))
    th = np.arctan2(np.sin(a), 3 + np.cos(a))
    assert np.allclose(quat[0, 0], [np.cos(th / 2), 0, 0, np.sin(th / 2)], rtol=0, atol=1e-15) and fb[0] == 0
    assert np.allclose(dst[0, 3:], [1 + 0.5 * np.cos(th), 2 + 0.5 * np.sin(th), 3], rtol=0, atol=1e-15)
    # I and a half turn about z at equal weight: no mean -- the first entry, one fallback; at 2 : 3 the heavier one, none
    half = np.diag([-1.0, -1.0, 1.0])
    _, quat, _, _, fb = _one_bone([np.eye(3), half], (2, 2))
    assert quat[0, 0].tolist() == [1, 0, 0, 0] and fb[0] == 1
    _, quat, _, _, fb = _one_bone([half, np.eye(3)], (2, 2))
    assert quat[0, 0].tolist() == [0, 0, 0, 1] and fb[0] == 1
    _, quat, _, _, fb = _one_bone([np.eye(3), half], (2, 3))
    assert np.allclose(quat[0, 0], [0, 0, 0, 1], rtol=0, atol=1e-15) and fb[0] == 0
    # a single entry: its row bit for bit (a row that is NOT what the rotation would lay), its quaternion, no spread
    row = np.array([[0.25, -1.0, 2.0, 7.0, 7.0, 7.0]])
    dst, quat, spr, rspr, fb = _one_bone([_rz(a)], (5,), src=row)
    assert np.array_equal(dst[0], row[0]) and spr[0] == 0.0 and rspr[0] == 0.0 and fb[0] == 0
    assert np.allclose(quat[0, 0], [np.cos(a / 2), 0, 0, np.sin(a / 2)], rtol=0, atol=1e-15)
    # an empty cover, and one whose only entry lies outside the source: zeros
    src, q, Rh = np.ones((1, 6)), np.eye(3).reshape(1, 1, 9), np.eye(3).reshape(1, 9)
    out = rref.blend_rot(src, q, Rh, np.array([0, 0, 1], np.int64), np.array([4], np.int32), np.array([1], np.float32), ((1, 0),), (0,),
                         np.array([[0.5, 0, 0]]))
    assert all(not np.asarray(o).any() for o in out)


def test_the_restatement_lays_a_chain_by_hand():
    """0 -> 1 -> 2 with rest bones x and 2 y.  Both windows turn bone 0 by a quarter turn about z (x -> y); bone 1 is turned by a quarter
    turn about x in one window and not at all in the other, at equal weight: its mean is an eighth turn about x, 2 y -> sqrt 2 (y + z)."""
    qz, qx = _rz(np.pi / 2), np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])
    body = np.array([[1.0, 0, 0], [0, 2.0, 0]])
    q = np.stack([np.stack([qz, np.eye(3)]), np.stack([qz, qx])]).reshape(2, 2, 9)
    Rh = np.tile(np.eye(3).reshape(9), (2, 1))
    roots = np.array([[1.0, 1, 1], [3.0, 1, 1]])
    src = np.zeros((2, 3, 3))
    for r in range(2):
        src[r, 0] = roots[r]
        src[r, 1] = src[r, 0] + q[r, 0].reshape(3, 3) @ body[0]
        src[r, 2] = src[r, 1] + q[r, 1].reshape(3, 3) @ body[1]
    dst, quat, spr, rspr, fb = rref.blend_rot(src.reshape(2, 9), q, Rh, np.array([0, 2], np.int64), np.array([0, 1], np.int32),
                                              np.array([1, 1], np.float32), ((1, 0), (2, 1)), (0, 1), body)
    r2 = np.sqrt(2.0)
    assert np.allclose(dst[0], [2, 1, 1, 2, 2, 1, 2, 2 + r2, 1 + r2], rtol=0, atol=1e-14) and fb[0] == 0
    assert np.allclose(quat[0], [[np.cos(np.pi / 4), 0, 0, np.sin(np.pi / 4)], [np.cos(np.pi / 8), np.sin(np.pi / 8), 0, 0]], rtol=0, atol=1e-15)
    # bone 0: both windows on the mean; bone 1: both an eighth turn (pi / 4) from it; over NB = 2 bones and W = 2
    assert np.isclose(rspr[0], np.sqrt(((np.pi / 4) ** 2 * 2) / (2 * 2.0)), rtol=1e-13)
    # the helper that rebuilds positions from the quaternions alone gives the same joints
    again = rref.fk_from_quaternions(dst.reshape(1, 3, 3), quat, ((1, 0), (2, 1)), body)
    assert np.allclose(again.reshape(1, 9), dst, rtol=0, atol=1e-14)


def test_rigid_rows_are_what_the_kernel_tests_need():
    rng = np.random.default_rng(3)
    u = rng.normal(size=(14, 3))
    body = (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.05, 0.55, (14, 1))).astype(np.float32)
    src, q, Rh = rref.rigid_rows(rng, 40, 15, rref.UPPER_WALK, rref.ROT_UPPER, 14, body)
    assert src.dtype == q.dtype == Rh.dtype == np.float32 and src.shape == (40, 45) and q.shape == (40, 14, 9) and Rh.shape == (40, 9)
    assert np.abs(src).max() < 8.0
    R = Rh.astype(np.float64).reshape(40, 3, 3)
    assert np.all(np.linalg.det(R) > 0.999) and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    # every row's joints are the forward kinematics of its own world rotations Rh^T q
    x = src.astype(np.float64).reshape(40, 15, 3)
    for b, (c, p) in enumerate(rref.UPPER_WALK):
        A = R.transpose(0, 2, 1) @ q.astype(np.float64).reshape(40, 14, 3, 3)[:, rref.ROT_UPPER[b]]
        assert np.abs(x[:, c] - x[:, p] - A @ body[b].astype(np.float64)).max() < 2e-6
    gaps = []
    off = np.arange(0, 41, 8).astype(np.int64)
    rref.blend_rot(src, q, Rh, off, np.arange(40, dtype=np.int32), rng.integers(1, 11, 40).astype(np.float32), rref.UPPER_WALK,
                   rref.ROT_UPPER, body, min_gap=gaps)
    assert len(gaps) == 5 * 14 and min(gaps) >= 1.0
