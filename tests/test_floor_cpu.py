"""CPU: the loader's floor views (PosePC.frame_ground_ / frame_contact_) on the stored frames of tests/golden/g11_loader.npz, the --floor
flags on the command line (defaults, refusals, what reaches ConfigDemo), the check of dense_infer's floor argument, the summary's
arithmetic, the two entry points' declarations, and the properties of the float64 restatement tests/floor_ref.py that the GPU tests
hold the kernels to."""
import numpy as np
import pytest

import floor_ref as fref
import main as cli
from conftest import golden
from test_data_cpu import _mat_tree


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    from mmego_amd.data import PosePC
    g = golden("g11_loader.npz")
    root = str(tmp_path_factory.mktemp("floor") / "Sample_data")
    _mat_tree(root, g)
    np.random.seed(0)
    ds = PosePC(train=False, vis=True, batch_length=20, root=root)
    return g, ds


def _stored(g):
    """-> (frame numbers in the loader's arrays of the fully stored frames, their planes [n, 4], their flags [n, 2])."""
    npts, full = g["mat.npts"].astype(np.int64), [int(i) for i in g["mat.full"]]
    number = np.cumsum(npts > 0) - 1                    # (the loader skips a frame without points)
    assert (npts[full] > 0).all()
    ground = np.asarray(g["mat.abcd_ground_2"], dtype=np.float32).reshape(len(full), 4)
    ground = np.where(ground[:, :1] > 0, -ground, ground)          # the loader's sign rule
    return number[full], ground, np.asarray(g["mat.foot_contact"]).reshape(len(full), 2)


def test_loader_views(loaded):
    g, ds = loaded
    F = len(ds.frame_npts_)
    assert ds.frame_ground_.shape == (F, 4) and ds.frame_ground_.dtype == np.float32
    assert ds.frame_contact_.shape == (F, 2) and ds.frame_contact_.dtype == np.uint8
    at, ground, flags = _stored(g)
    assert len(at) == 21
    assert np.array_equal(ds.frame_ground_[at], ground)
    assert np.array_equal(ds.frame_contact_[at], (flags != 0).astype(np.uint8)) and set(np.unique(ds.frame_contact_)) <= {0, 1}
    # what the loader hands out in the reference's tuple order is the same data: window 0 is the recording's last 20 frames
    assert np.array_equal(np.asarray(ds.ground_[0], dtype=np.float32).reshape(20, 4), ds.frame_ground_[-20:])
    assert np.array_equal(np.asarray(ds.foot_contact_[0])[:, :, 1], ds.frame_contact_[-20:])


def test_flag_columns_belong_to_joints_15_and_19(loaded):
    """In float64 on the stored frames: every flagged foot lies under 6 cm (the highest at 5.2), every unflagged one above 8 (the lowest
    at 8.1); with the columns swapped, or other joints, that does not hold."""
    g, ds = loaded
    at, _, _ = _stored(g)
    gr = ds.frame_ground_[at].astype(np.float64)
    assert np.abs(np.linalg.norm(gr[:, :3], axis=1) - 1.0).max() < 1e-6
    feet = np.asarray(ds.frame_key_, dtype=np.float64)[at][:, [15, 19]]
    h = np.einsum("fki,fi->fk", feet, gr[:, :3]) + gr[:, 3:4]
    c = ds.frame_contact_[at] != 0
    print("flagged feet: %.4f .. %.4f m; unflagged: %.4f .. m" % (h[c].min(), h[c].max(), h[~c].min()))
    assert c.any() and (~c).any()
    assert (h[c] < 0.06).all() and (h[~c] > 0.08).all()
    assert not ((h[c[:, ::-1]] < 0.06).all() and (h[~c[:, ::-1]] > 0.08).all()), "the swapped columns would not separate"


def test_the_views_leave_the_loader_as_it_was(loaded):
    g, ds = loaded
    real = golden("real16.npz")
    assert np.array_equal(ds.data_ti_[0], real["x"][0]), "window 0 under the same seed: the views drew nothing"
    assert np.array_equal(ds.data_key_[0].astype(np.float32), real["target"][0])
    assert len(ds[0]) == 9 and len(ds._items) == 9


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_floor_reaches_the_config_and_is_off_by_default():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "upper_variant", "metrics", "smooth", "floor")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    assert ConfigDemo.floor is None
    try:
        for argv, want in ((["--infer", "--dense", "--floor", "measure"], ("measure", 6.0, 0.0)),
                           (["--infer", "--dense", "--floor", "clamp", "--floor_margin_cm", "1.5"], ("clamp", 6.0, 1.5)),
                           (["--infer", "--dense", "--floor", "clamp", "--floor_contact_cm", "4", "--blend_space", "bones"], ("clamp", 4.0, 0.0)),
                           (["--infer", "--dense", "--floor", "measure", "--blend_space", "rot"], ("measure", 6.0, 0.0)),
                           (["--infer", "--dense", "--smooth", "2"], None), (["--infer"], None)):
            args = p.parse_args(argv)
            cli.check_dense(p, args)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert ConfigDemo.floor == want, argv
    finally:
        for c, k, v in keep:
            if v is not missing:
                setattr(c, k, v)
            elif k in c.__dict__:
                delattr(c, k)


@pytest.mark.parametrize("flag", [["--floor", "measure"], ["--floor_contact_cm", "5"], ["--floor_margin_cm", "1"]])
def test_the_floor_flags_need_dense(capsys, monkeypatch, flag):
    for head in (["--infer"], ["--train", "--network", "Upper_Net"], []):
        assert "%s belongs to --infer --dense" % flag[0] in _refused(head + flag, capsys, monkeypatch), head


@pytest.mark.parametrize("flag", [["--floor_contact_cm", "5"], ["--floor_margin_cm", "1"]])
def test_heights_need_floor(capsys, monkeypatch, flag):
    assert "%s belongs to --floor" % flag[0] in _refused(["--infer", "--dense"] + flag, capsys, monkeypatch)


def test_other_values_are_refused(capsys, monkeypatch):
    head = ["--infer", "--dense"]
    assert "--floor clamp does not go with --blend_space rot" in _refused(head + ["--floor", "clamp", "--blend_space", "rot"], capsys, monkeypatch)
    assert "invalid choice" in _refused(head + ["--floor", "snap"], capsys, monkeypatch)
    for bad in ("0", "-1", "nan", "inf"):
        assert "--floor_contact_cm is a height" in _refused(head + ["--floor", "measure", "--floor_contact_cm", bad], capsys, monkeypatch)
    for bad in ("-0.5", "nan", "inf"):
        assert "--floor_margin_cm is a height" in _refused(head + ["--floor", "clamp", "--floor_margin_cm", bad], capsys, monkeypatch)


def test_the_floor_argument_is_checked():
    from mmego_amd import dense
    assert dense._check_floor(None) is None
    assert dense._check_floor(("clamp", 6, np.float32(0.5))) == ("clamp", 6.0, 0.5)
    for bad in (("clamp", 6), ("snap", 6, 0), ("measure", 0, 0), ("measure", -1, 0), ("measure", 6, -1), ("measure", float("nan"), 0),
                ("measure", 6, float("inf")), ("measure", True, 0), ("measure", "6", 0), "measure"):
        with pytest.raises(ValueError, match="floor"):
            dense._check_floor(bad)


def test_summary_arithmetic():
    from mmego_amd import dense
    sums = np.zeros(22)
    sums[:11] = [0.30, 0.04, 2, 5, 4, 6, 0.12, 0.01, 1, 6, 5]          # foot 0 over 10 rows
    sums[11:] = [0.10, 0.00, 0, 0, 0, 0, 0.00, 0.00, 0, 0, 0]          # foot 1: nothing penetrates, nothing low, nothing flagged
    s = dense._floor_summary(sums, 10, "x_", target=True)
    assert s["x_foot_height_err_cm_per_foot"] == (pytest.approx(3.0), pytest.approx(1.0)) and s["x_foot_height_err_cm"] == pytest.approx(2.0)
    assert s["x_penetration_rate_per_foot"] == (0.2, 0.0) and s["x_penetration_rate"] == 0.1
    assert s["x_penetration_cm_per_foot"] == (pytest.approx(2.0), None) and s["x_penetration_cm"] == pytest.approx(2.0)
    assert s["x_contact_precision_per_foot"] == (0.8, None) and s["x_contact_recall_per_foot"] == (pytest.approx(4 / 6), None)
    assert s["x_hover_cm_per_foot"] == (pytest.approx(2.0), None)
    assert s["target_penetration_rate"] == 0.05 and s["target_penetration_cm"] == pytest.approx(1.0)
    assert s["target_contact_precision"] == pytest.approx(5 / 6) and s["target_contact_recall"] == pytest.approx(5 / 6)
    assert not any(k.startswith("target_") for k in dense._floor_summary(sums, 10, "single_"))
    assert set(dense._floor_summary(sums, 10)) == {k + t for k in dense.FLOOR_KEYS for t in ("", "_per_foot")}


def test_the_entry_points_are_declared_as_ops_calls_them():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_floor_stats"]] == ["stream", "lo", "ldl", "tgt", "ldt", "ground", "contact", "seg", "rows", "H", "out"]
    assert [n for _, n in protos["mmego_floor_clamp"]] == ["stream", "src", "lds", "ground", "seg", "rows", "margin", "dst", "ldd", "lifted",
                                                           "fallback"]
    assert callable(ops.floor_stats) and callable(ops.floor_clamp) and ops.FLOOR_W == fref.FLOOR_W == 22


@pytest.mark.parametrize("margin", [0.0, 0.02])
def test_properties_of_the_restatement(margin):
    """2 000 random rows (4 000 legs): bone lengths kept to 1e-12, the foot bone's vector kept, ankle and foot at or above the margin,
    legs that were above it identical."""
    rows, ground = fref.random_legs(np.random.default_rng(5), 2000)
    seg = np.zeros(len(rows), dtype=np.int32)
    dst, lifted, fallback, legs = fref.clamp(rows, ground, seg, margin)
    x, y = rows.reshape(-1, 8, 3), dst.reshape(-1, 8, 3)
    n_lifted = 0
    for r in range(len(x)):
        pl = fref.plane(ground[r])
        for (h, k, a, t), res in zip(fref.LEGS, legs[r]):
            assert np.array_equal(y[r, h], x[r, h])
            if res["lift"] == 0.0:
                assert np.array_equal(y[r, [k, a, t]], x[r, [k, a, t]]) and res["fallback"] == 0
                assert fref.height(pl, x[r, t]) >= margin and fref.height(pl, x[r, a]) >= margin
                continue
            n_lifted += 1
            assert res["fallback"] == 0, "this draw has no leg out of reach"
            assert abs(np.linalg.norm(y[r, k] - y[r, h]) - np.linalg.norm(x[r, k] - x[r, h])) <= 1e-12
            assert abs(np.linalg.norm(y[r, a] - y[r, k]) - np.linalg.norm(x[r, a] - x[r, k])) <= 1e-12
            assert np.abs((y[r, t] - y[r, a]) - (x[r, t] - x[r, a])).max() <= 1e-15
            assert fref.height(pl, y[r, a]) >= margin - 1e-12 and fref.height(pl, y[r, t]) >= margin - 1e-12
            assert abs(min(fref.height(pl, y[r, a]), fref.height(pl, y[r, t])) - margin) <= 1e-12, "no higher than needed"
            assert abs(fref.height(pl, y[r, a]) - fref.height(pl, x[r, a]) - res["lift"]) <= 1e-12
    print("margin %g: %d of %d legs lifted, largest lift %.3f m" % (margin, n_lifted, 2 * len(x), lifted.max()))
    assert 0.15 * 2 * len(x) <= n_lifted <= 0.7 * 2 * len(x) and not fallback.any()
    assert np.array_equal(lifted > 0, [any(res["lift"] > 0 for res in both) for both in legs])


def test_built_legs_of_the_restatement():
    """A target out of reach lands at reach along u and counts; a straight vertical leg bends to the foot's side; with a vertical foot
    bone, to the coordinate axis; rows outside a segment and rows without a plane are copies."""
    up = (np.array([0.0, 0.0, 1.0]), 0.0)
    Hp, K, A, T = np.array([0.0, 0.0, -1.0]), np.array([0.0, 0.1, -1.4]), np.array([0.0, 0.0, -1.8]), np.array([0.1, 0.0, -1.85])
    res = fref.leg(Hp, K, A, T, up, 0.0)
    l1, l2 = np.linalg.norm(K - Hp), np.linalg.norm(A - K)
    assert res["fallback"] == 1 and res["lift"] == pytest.approx(1.85)
    assert np.linalg.norm(res["A"] - Hp) == pytest.approx((l1 + l2) * (1 - 1e-6), abs=1e-12) and res["A"][2] > Hp[2]
    Hp, K, A, T = np.array([0.0, 0.0, 0.9]), np.array([0.0, 0.0, 0.5]), np.array([0.0, 0.0, 0.1]), np.array([0.1, 0.0, -0.05])
    res = fref.leg(Hp, K, A, T, up, 0.0)
    assert res["fallback"] == 0 and res["K"][0] > 0.05 and abs(res["K"][1]) < 1e-15, "the knee goes where the foot points"
    assert np.linalg.norm(res["K"] - Hp) == pytest.approx(0.4, abs=1e-12) and np.linalg.norm(res["A"] - res["K"]) == pytest.approx(0.4, abs=1e-12)
    res = fref.leg(Hp, K, A, np.array([0.0, 0.0, -0.05]), up, 0.0)
    assert res["fallback"] == 0 and res["K"][0] > 0.05 and abs(res["K"][1]) < 1e-15, "the first axis of the smallest |u_i|: x"
    assert np.isfinite(res["K"]).all() and np.linalg.norm(res["K"] - Hp) == pytest.approx(0.4, abs=1e-12)
    rows, ground = fref.random_legs(np.random.default_rng(1), 3)
    ground[:] = [0.0, 0.0, 1.0, -0.5]
    ground[2, :3] = 0.0
    dst, lifted, fallback, _ = fref.clamp(rows, ground, np.array([0, -1, 0], dtype=np.int32), 0.0)
    assert lifted[0] > 0 and np.array_equal(dst[1:], rows[1:]) and list(lifted[1:]) == [0, 0] and list(fallback) == [0, 0, 2]
