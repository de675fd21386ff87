"""CPU: --blend_space on the command line, the walk tables of the bone-length-preserving blend (mmego_amd/skeleton.py), the host checks
ops.blend_bones makes before it launches, the two entry points' declarations, and the restatement of tests/bone_blend_ref.py on cases
worked out by hand."""
import numpy as np
import pytest

import bone_blend_ref as bref
import main as cli


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_blend_space_reaches_the_config():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "upper_variant", "metrics")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    assert ConfigDemo.blend_space is None
    try:
        for argv, want in ((["--infer", "--dense", "--blend_space", "bones"], "bones"),
                           (["--infer", "--dense", "--stride", "3", "--blend_space", "joints"], "joints"),
                           (["--infer", "--dense"], None), (["--infer"], None)):
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


@pytest.mark.parametrize("value", ["bones", "joints"])
def test_blend_space_needs_dense(capsys, monkeypatch, value):
    for head in (["--infer"], ["--train", "--network", "Upper_Net"], []):
        err = _refused(head + ["--blend_space", value], capsys, monkeypatch)
        assert "--blend_space belongs to --infer --dense" in err, head


def test_a_third_blend_space_is_refused(capsys, monkeypatch):
    assert "invalid choice" in _refused(["--infer", "--dense", "--blend_space", "rotations"], capsys, monkeypatch)


def test_walk_tables_go_parents_first():
    from mmego_amd import skeleton
    for walk, joint_map, roots, rows, nb in ((skeleton.WALK_UPPER, skeleton.UPPER_MAP, [20], skeleton.WALK_UPPER_ROWS, 14),
                                             (skeleton.WALK_LOWER, skeleton.LOWER_MAP, [12, 16], skeleton.WALK_LOWER_ROWS, 6)):
        J = len(joint_map)
        assert walk.shape == (nb, 2) and walk.dtype == np.int32 and walk.min() >= 0 and walk.max() < J
        children = walk[:, 0].tolist()
        assert len(set(children)) == nb, "every joint is a child at most once"
        assert sorted(joint_map[j] for j in range(J) if j not in children) == roots
        placed = set(range(J)) - set(children)
        for c, p in walk.tolist():
            assert p in placed, "bone (%d, %d) comes before its parent's" % (c, p)
            placed.add(c)
        assert placed == set(range(J))
    assert skeleton.WALK_UPPER_ROWS == tuple(range(14)) and skeleton.WALK_LOWER_ROWS == tuple(range(14, 20))
    # in the 21-joint numbering they are the reference's bone lists, (parent, child) turned round
    assert [[skeleton.UPPER_MAP[p], skeleton.UPPER_MAP[c]] for c, p in skeleton.WALK_UPPER.tolist()] == skeleton.BONES_UPPER
    assert [[skeleton.LOWER_MAP[p], skeleton.LOWER_MAP[c]] for c, p in skeleton.WALK_LOWER.tolist()] == skeleton.BONES_LOWER
    # and the tables the test helper spells out by hand
    assert skeleton.WALK_UPPER.tolist() == [list(b) for b in bref.UPPER_WALK] and skeleton.WALK_LOWER.tolist() == [list(b) for b in bref.LOWER_WALK]


def test_the_entry_points_are_declared_as_ops_calls_them():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_blend_bones"]] == ["stream", "src", "nrows", "J", "cov_off", "cov_row", "cov_w", "F", "bones",
                                                           "bone_len", "NB", "dst", "ldd", "spread", "fallback"]
    assert [n for _, n in protos["mmego_bone_length_dev"]] == ["stream", "X", "ldx", "n", "J", "bones", "bone_len", "NB", "out", "ldo"]
    assert callable(ops.blend_bones) and callable(ops.bone_length_dev) and ops.BONES_MAX_J == 21


def test_the_bone_list_is_checked_on_the_host():
    from mmego_amd import ops, skeleton
    L = np.full(14, 0.3, np.float32)
    b, l, nb = ops._bones_on(skeleton.WALK_UPPER, L, 15, "cpu", "t")
    assert nb == 14 and b.dtype == __import__("torch").int32 and tuple(b.shape) == (14, 2) and tuple(l.shape) == (14,)
    assert ops._bones_on([], [], 1, "cpu", "t")[2] == 0                                  # one joint, no bone
    twice = skeleton.WALK_UPPER.copy()
    twice[5] = (3, 4)
    late = skeleton.WALK_UPPER[[1, 0] + list(range(2, 14))]
    with pytest.raises(ValueError, match="child of two bones"):
        ops._bones_on(twice, L, 15, "cpu", "t")
    with pytest.raises(ValueError, match="parents first"):
        ops._bones_on(late, L, 15, "cpu", "t")
    with pytest.raises(ValueError, match="parents first"):
        ops._bones_on([(0, 1), (1, 2), (2, 0)], L[:3], 4, "cpu", "t")                   # a cycle has no root to start from
    with pytest.raises(ValueError, match="parents first"):
        ops._bones_on([(1, 1)], L[:1], 2, "cpu", "t")
    with pytest.raises(IndexError):
        ops._bones_on([(1, 15)], L[:1], 15, "cpu", "t")
    with pytest.raises(ValueError, match="at most one bone less"):
        ops._bones_on(skeleton.WALK_UPPER, L, 14, "cpu", "t")
    for bad in (0.0, -0.1, np.nan, np.inf):
        Lb = L.copy()
        Lb[7] = bad
        with pytest.raises(ValueError, match="finite and positive"):
            ops._bones_on(skeleton.WALK_UPPER, Lb, 15, "cpu", "t")
    with pytest.raises(ValueError, match="one length per bone"):
        ops._bones_on(skeleton.WALK_UPPER, L[:13], 15, "cpu", "t")


def test_bone_lengths_of_the_bone_set():
    from mmego_amd import dense
    rng = np.random.default_rng(0)
    body = rng.normal(0, 0.3, (20, 3)).astype(np.float32)
    up, lo = dense.bone_lengths(body)
    want = np.sqrt((body.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    assert up.dtype == np.float32 and np.array_equal(up, want[:14]) and np.array_equal(lo, want[14:])


def test_the_restatement_on_cases_worked_by_hand():
    """A chain 0 -> 1 -> 2 of lengths 1 and 2.  Two windows see bone 0 along x and along y: the blend lies along the diagonal at length
    1, where the vector mean is 1 / sqrt(2) long; bone 1 along z in both: it hangs 2 below the blended joint."""
    bones, L = ((1, 0), (2, 1)), np.array([1.0, 2.0], np.float32)
    src = np.array([[0, 0, 0, 1, 0, 0, 1, 0, 2], [2, 0, 0, 2, 1, 0, 2, 1, 2], [5, 5, 5, 5, 5, 5, 5, 5, 5]], dtype=np.float32)
    off = np.array([0, 0, 1, 3, 5, 7], np.int64)
    row = np.array([1, 0, 1, 0, 7, 2, 2], np.int32)                   # frame 3: one of its two rows lies outside the source
    w = np.array([3, 1, 1, 2, 5, 1, 4], np.float32)
    dst, spr, fb = bref.blend_bones(src, off, row, w, bones, L)
    r = np.sqrt(0.5)
    assert not dst[0].any() and spr[0] == 0.0
    assert np.array_equal(dst[1], src[1]) and spr[1] == 0.0
    assert np.allclose(dst[2], [1, 0, 0, 1 + r, r, 0, 1 + r, r, 2], rtol=0, atol=1e-15)
    assert np.array_equal(dst[3], src[0]) and spr[3] == 0.0
    d = np.stack([src[0], src[1]]).astype(np.float64).reshape(2, 3, 3) - dst[2].reshape(3, 3)
    assert np.isclose(spr[2], np.sqrt((d ** 2).sum() / (3 * 2.0)), rtol=1e-14)
    # frame 4: the same degenerate row twice -- both bones fall back and, their differences being zero, stay on the parent
    assert np.array_equal(dst[4], src[2]) and fb.tolist() == [0, 0, 0, 0, 2]
    assert np.allclose(bref.bone_lengths(dst[[1, 2, 3]], bones), [[1, 2]] * 3, rtol=0, atol=1e-15)
    assert np.allclose(bref.bone_length_dev(dst[[2, 4]], bones, L), [[0, 0], [1, 2]], rtol=0, atol=1e-15)
    # exactly opposite differences at equal weights: the first entry's direction; the heavier entry's at unequal ones
    src = np.array([[0, 0, 0, 0.25, 0, 0], [0, 0, 0, -0.25, 0, 0]], dtype=np.float32)
    for wts, x, n in (((2, 2), 0.25, 1), ((2, 3), -0.25, 0), ((3, 2), 0.25, 0)):
        dst, _, fb = bref.blend_bones(src, np.array([0, 2], np.int64), np.array([0, 1], np.int32), np.asarray(wts, np.float32), ((1, 0),),
                                      np.array([0.25], np.float32))
        assert dst[0].tolist() == [0, 0, 0, x, 0, 0] and fb[0] == n, wts
