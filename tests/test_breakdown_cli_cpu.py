"""CPU: --breakdown on the command line (refusals, acceptances, what reaches ConfigDemo), the (bin_cm, nbins) argument's check, the host
helpers evaluation.hist_quantile / pck_auc against numpy on hand-made histograms, the loader's per-recording arrays on a small synthetic
tree, and the two entry points' declarations."""
import os

import numpy as np
import pytest
import scipy.io as scio

import breakdown_ref as ref
import main as cli


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_breakdown_reaches_the_config_and_is_off_by_default():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "upper_variant", "metrics", "smooth", "rot_smooth",
             "floor", "breakdown", "gt_head_pose", "pose_noise_deg", "pose_noise_t")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    assert not getattr(ConfigDemo, "breakdown", False)
    try:
        for argv, want in ((["--infer", "--breakdown"], True), (["--infer", "--dense", "--breakdown"], True),
                           (["--infer", "--breakdown", "--metrics", "full", "--gt_head_pose"], True),
                           (["--infer", "--dense", "--breakdown", "--stride", "3", "--blend", "triangle", "--blend_space", "bones", "--smooth", "4",
                             "--floor", "clamp", "--save_pred", "x.npz", "--metrics", "full"], True),
                           (["--infer", "--dense", "--breakdown", "--blend_space", "rot", "--rot_smooth", "3", "--floor", "measure"], True),
                           (["--infer", "--breakdown", "--pose_noise_deg", "1.0", "--seed", "2"], True),
                           (["--infer", "--breakdown", "--network", "Lower_Net"], True),
                           (["--infer", "--dense"], False), (["--infer"], False)):
            args = p.parse_args(argv)
            cli.check_breakdown(p, args)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert ConfigDemo.breakdown is want, argv
    finally:
        for c, k, v in keep:                         # (what the class itself held; what it inherits comes back by deleting the override)
            if v is not missing:
                setattr(c, k, v)
            elif k in c.__dict__:
                delattr(c, k)
    assert p.parse_args(["--infer"]).breakdown is False


def test_breakdown_is_refused_outside_an_inference_pass(capsys, monkeypatch):
    assert "--breakdown goes with --infer only" in _refused(["--breakdown"], capsys, monkeypatch)
    for net in ("IMU_Net", "Upper_Net", "Lower_Net"):
        assert "--breakdown does not go with --train" in _refused(["--train", "--network", net, "--breakdown"], capsys, monkeypatch)
    assert "--breakdown does not go with --train" in _refused(["--train", "--infer", "--network", "Upper_Net", "--breakdown"], capsys, monkeypatch)
    assert "--breakdown does not go with --vis" in _refused(["--infer", "--vis", "--breakdown"], capsys, monkeypatch)
    assert "--breakdown does not go with --network IMU_Net" in _refused(["--infer", "--network", "IMU_Net", "--breakdown"], capsys, monkeypatch)
    assert "expected" not in _refused(["--breakdown"], capsys, monkeypatch)          # (a store_true flag: it takes no value)


def test_the_breakdown_argument_is_checked():
    from mmego_amd import evaluation as ev
    assert ev.BREAKDOWN_BINS == (0.05, 4096) and ev.check_breakdown(ev.BREAKDOWN_BINS) == (0.05, 4096)
    assert np.float32(100.0 / ev.BREAKDOWN_BINS[0]) == np.float32(2000.0) and 100.0 / ev.BREAKDOWN_BINS[0] == 2000.0
    assert ev.check_breakdown(None) is None
    assert ev.check_breakdown((np.float64(0.5), np.int64(2))) == (0.5, 2) and ev.check_breakdown([1, 300]) == (1.0, 300)
    for bad in ((0.05,), (0.05, 4096, 1), 0.05, "0.05", (0.0, 64), (-0.5, 64), (float("nan"), 64), (float("inf"), 64), (True, 64), ("0.5", 64),
                (0.5, 1), (0.5, 0), (0.5, 4097), (0.5, 64.0), (0.5, True), (0.3, 64), (0.07, 64), (1e-60, 64)):
        with pytest.raises(ValueError, match="breakdown"):
            ev.check_breakdown(bad)


def _np_quantile(values, q, width, nbins):
    """What hist_quantile promises about raw values: within one bin width of x_(ceil(q n)) where that lies below the overflow bin."""
    return ref.order_statistic(values, q)


def test_hist_quantile_and_pck_auc_on_hand_made_histograms():
    from mmego_amd import evaluation as ev
    # empty
    assert ev.hist_quantile(np.zeros(8, np.int64), 0.5, 0.5) == (None, False) and ev.pck_auc(np.zeros(8, np.int64), 0.5) is None
    # all mass in one bin: every quantile interpolates across that bin
    h = np.zeros(10, np.int64)
    h[3] = 40
    for q in (0.01, 0.5, 0.9, 1.0):
        v, clipped = ev.hist_quantile(h, 0.5, q)
        assert not clipped and v == pytest.approx((3 + q) * 0.5, abs=1e-12)
    # by hand: counts 2, 0, 6, 2 | overflow 0; bins 1 cm wide
    h = np.asarray([2, 0, 6, 2, 0])
    assert ev.hist_quantile(h, 1.0, 0.2) == (pytest.approx(1.0), False)              # q n = 2 = cum[0]: the top of bin 0
    assert ev.hist_quantile(h, 1.0, 0.5) == (pytest.approx(2.5), False)              # q n = 5: 3 of bin 2's 6 values
    assert ev.hist_quantile(h, 1.0, 0.9) == (pytest.approx(3.5), False)
    assert ev.hist_quantile(h, 1.0, 1.0) == (pytest.approx(4.0), False)
    assert ev.pck_auc(h, 1.0, upto_cm=3.0) == pytest.approx((0.2 + 0.2 + 0.8) / 3)  # PCK at the edges 1, 2, 3 cm
    assert ev.pck_auc(h, 1.0, upto_cm=15.0) == pytest.approx((0.2 + 0.2 + 0.8 + 1.0) / 4)    # (edges of regular bins only: k <= nbins - 1)
    assert ev.pck_auc(h, 1.0, upto_cm=0.5) is None
    # a quantile landing in the overflow bin: its lower edge, flagged
    h = np.asarray([5, 3, 0, 2])
    assert ev.hist_quantile(h, 2.0, 0.5) == (pytest.approx(2.0), False)
    assert ev.hist_quantile(h, 2.0, 0.9) == (6.0, True) and ev.hist_quantile(h, 2.0, 0.81) == (6.0, True)
    assert ev.hist_quantile(h, 2.0, 0.8) == (pytest.approx(4.0), False)
    for q in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ev.hist_quantile(h, 2.0, q)
    # random values: against numpy's order statistic, within a bin width; pck_auc against the restatement exactly
    rng = np.random.default_rng(5)
    x = rng.gamma(2.0, 3.0, 5000)
    width, nbins = 0.05, 4096
    h = np.bincount(np.minimum((x / width).astype(np.int64), nbins - 1), minlength=nbins)
    for q in (0.5, 0.9, 0.95, 0.99, 1.0):
        v, clipped = ev.hist_quantile(h, width, q)
        assert not clipped and abs(v - _np_quantile(x, q, width, nbins)) <= width
    assert ev.pck_auc(h, width) == ref.pck_auc(h, width) and ev.pck_auc_edges(nbins, width) == 300
    direct = np.mean([(x < k * width).mean() for k in range(1, 301)])
    assert ev.pck_auc(h, width) == pytest.approx(direct, abs=1e-12)


def _make_tree(root, rng, layout):
    """layout: (action directory name, snippet directory name, frames) in any order."""
    for a, s, count in layout:
        d = os.path.join(root, a, s)
        os.makedirs(d)
        skel = rng.normal(0, 0.4, (32, 3))
        for f in range(count):
            n = int(rng.integers(3, 9))
            pc = np.concatenate([rng.normal(0, 0.4, (n, 3)), rng.uniform(10, 46, (n, 1)), rng.normal(0, 0.4, (n, 1))], 1)
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            imu = np.concatenate([np.tile(q.reshape(1, 9), (20, 1)), rng.normal(size=(20, 6))], 1)
            scio.savemat(os.path.join(d, "frame_%d.mat" % f), {
                "pc_xyziv_ti2": pc.astype(np.float32), "pc_xyz_key_2": skel + 0.01 * f, "imu_save_l": imu, "R_btc": q,
                "orientation_imu_img": np.eye(3), "t_R0R": rng.normal(size=(1, 3)), "abcd_ground_2": np.array([[0.0, 0.0, -1.0, 1.0]]),
                "foot_contact": np.array([[1, 0]])})


def test_the_loader_knows_every_recordings_action_and_every_windows_recording(tmp_path):
    from mmego_amd.data import DensePlan, PosePC, list_snippets
    root = str(tmp_path / "Sample_data")
    # directories 01, 03, 07 (non-consecutive numbers); 01/s0 is the very first snippet, which the loader skips as the reference does
    layout = [("01", "s0", 5), ("01", "s1", 9), ("03", "s0", 4), ("03", "s1", 2), ("03", "s2", 13), ("07", "s0", 8)]
    _make_tree(root, np.random.default_rng(1), layout)
    T = 4
    np.random.seed(0)
    vis = PosePC(train=False, vis=True, batch_length=T, root=root)
    snippets = list_snippets(root)
    assert [(a, j) for a, j, _ in snippets] == [(0, 1), (1, 0), (1, 1), (1, 2), (2, 0)]
    assert vis.rec_action_.tolist() == [1, 3, 3, 3, 7] and vis.rec_snippet_.tolist() == [1, 0, 1, 2, 0]
    assert vis.rec_action_.dtype == vis.rec_snippet_.dtype == vis.win_rec_.dtype == np.int64
    assert np.array_equal(np.bincount(vis.frame_rec_), [9, 4, 2, 13, 8])
    # windows: 2, 1, 0, 3, 2 per recording, in the recordings' order; every window's frames lie in its recording
    assert vis.win_rec_.tolist() == [0, 0, 1, 3, 3, 3, 4, 4] and len(vis.win_rec_) == len(vis.data_ti_) == len(vis.win_start_)
    assert np.array_equal(vis.frame_rec_[vis.win_start_], vis.win_rec_) and np.array_equal(vis.frame_rec_[vis.win_start_ + T - 1], vis.win_rec_)
    # a shuffled split permutes win_rec_ with the other window arrays
    np.random.seed(0)
    test = PosePC(train=False, vis=False, batch_length=T, root=root)
    assert sorted(test.win_rec_.tolist()) == vis.win_rec_.tolist() and test.win_rec_.tolist() != vis.win_rec_.tolist()
    assert np.array_equal(test.frame_rec_[test.win_start_], test.win_rec_)
    assert test.rec_action_.tolist() == vis.rec_action_.tolist()
    from mmego_amd.evaluation import dataset_groups
    win_rec, act, snip = dataset_groups(test)
    assert len(win_rec) == len(test) == 8 - int(8 * 0.8) and np.array_equal(win_rec, test.win_rec_[test.split_cut:])
    assert np.array_equal(dataset_groups(vis)[0], vis.win_rec_) and act.tolist() == [1, 3, 3, 3, 7] and snip.tolist() == [1, 0, 1, 2, 0]
    # the key skeleton of window i of the shuffled arrays is the one of its frames (the permutation moved them together)
    for i in range(len(test.win_rec_)):
        assert np.array_equal(np.asarray(test.data_key_[i]), np.asarray(test.frame_key_[test.win_start_[i]:test.win_start_[i] + T]))


def test_a_split_without_recordings_is_refused():
    from mmego_amd.data import ArraySplit
    from mmego_amd.evaluation import dataset_groups
    z = np.zeros((2, 1), dtype=np.float32)
    with pytest.raises(ValueError, match="breakdown"):
        dataset_groups(ArraySplit(z, z, z, z, z))


def test_the_entry_points_are_declared_as_ops_calls_them():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_colsum_groups"]] == ["stream", "X", "ldx", "rows", "C", "group", "G", "out", "ldo", "count"]
    assert [n for _, n in protos["mmego_hist_groups"]] == ["stream", "X", "ldx", "rows", "C", "group", "G", "inv_width", "nbins", "pool", "hist",
                                                          "dropped"]
    assert callable(ops.colsum_groups) and callable(ops.hist_groups)
    assert ops.GROUPS_MAX_G == 65535 and ops.GROUPS_MAX_ROWS == 1 << 24 and ops.HIST_MAX_BINS == 4096
