"""GPU: the error breakdown of the evaluation passes (dense.dense_infer and processors.evaluate_full under breakdown=(bin_cm, nbins),
`main.py --infer --dense --breakdown`) on the tiny synthetic Sample_data tree of tests/test_dense_infer_gpu.py extended to three
actions: 01 (s0, the skipped first snippet, and 23 frames), 02 (20 and 41 frames) and 05, which holds only a recording of 7 frames --
shorter than frame_no = 20, so the action has no covered frame and no window.  Nets from torch.manual_seed, the recorded head pose.

Every by_action / by_recording figure against a float64 recomputation from the pass's own predictions (1e-3 cm, the project's bar for
the error metric; 1e-3 deg for rot_deg); percentiles against the float64 order statistic x_(ceil(q n)) within two bin widths (both lie
in one bin, or in neighbouring bins where fp32 and float64 disagree about an edge, and the interpolation stays inside its bin)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.io as scio
import torch

import breakdown_ref as ref
import dense_ref
import pose_metrics_ref as pm
from conftest import ROOT

pytestmark = pytest.mark.gpu

T = 20
LAYOUT = ((1, 0, 2), (1, 1, 23), (2, 1, 20), (2, 2, 41), (5, 1, 7))           # (action, snippet, frames); the first is skipped by the loader
LENGTHS = (23, 20, 41, 7)
REC_ACTION, REC_SNIPPET = (1, 2, 2, 5), (1, 0, 1, 0)
ACTIONS = (1, 2, 5)
F = sum(LENGTHS)
# bins of 0.5 cm up to 2047.5 cm: seeded random nets can be a metre off, which --breakdown's own 0.05 cm x 4096 would put in the overflow
# bin; 100 / 0.5 = 200 bins per metre is a float32.  The tests assert on the float64 side that p99 lies below the overflow bin.
BINS = (0.5, 4096)
NEW_KEYS = {"by_action", "by_recording", "percentiles_cm", "percentile_clipped", "beyond", "per_joint_median_cm", "pck_auc", "breakdown",
            "joint_errors", "dropped", "error_hist"}
NUMBER = r"(?:[-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?|None|nan)"


def _make_dataset(root, rng):
    for a, s, count in LAYOUT:
        d = os.path.join(root, "%02d" % a, "s%d" % s)
        os.makedirs(d)
        skel = rng.normal(0, 0.4, (32, 3)) + np.array([0.8, 0.0, 0.2])
        for f in range(count):
            n = int(rng.integers(20, 150))
            pc = np.concatenate([rng.normal([0.8, 0.0, 0.2], 0.4, (n, 3)), rng.uniform(10, 46, (n, 1)), rng.normal(0, 0.4, (n, 1))], 1)
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            imu = np.concatenate([np.tile(q.reshape(1, 9), (20, 1)), rng.normal(size=(20, 6))], 1)
            scio.savemat(os.path.join(d, "frame_%d.mat" % f), {
                "pc_xyziv_ti2": pc.astype(np.float32), "pc_xyz_key_2": skel + rng.normal(0, 0.05, (32, 3)) + 0.01 * f,
                "imu_save_l": imu, "R_btc": q, "orientation_imu_img": np.eye(3), "t_R0R": rng.normal(size=(1, 3)),
                "abcd_ground_2": np.array([[0.0, 0.0, -1.0, 1.0]]), "foot_contact": np.array([[1, 0]])})


class _World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The tree, its PosePC with the per-frame clouds, seeded nets, and the passes the tests share (each computed once)."""
    assert torch.cuda.is_available()
    from mmego_amd import dense, nets, processors
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import PosePC
    w = _World()
    w.tmp = tmp_path_factory.mktemp("breakdown")
    w.data = str(w.tmp / "Sample_data")
    _make_dataset(w.data, np.random.default_rng(0))
    np.random.seed(3)
    w.ds = PosePC(train=False, vis=True, keep_frames=True, batch_length=T, root=w.data)
    assert len(w.ds.frame_npts_) == F and len(w.ds) == 4
    assert w.ds.rec_action_.tolist() == list(REC_ACTION) and w.ds.rec_snippet_.tolist() == list(REC_SNIPPET)
    keep = ConfigDemo.gt_head_pose
    ConfigDemo.gt_head_pose = True
    try:
        w.base = processors._Base(ConfigDemo, make_dirs=False)
    finally:
        ConfigDemo.gt_head_pose = keep
    w.dev = w.base.device
    torch.manual_seed(0)
    w.up, w.lo = nets.UpperNet().to(w.dev).eval(), nets.LowerNet(64).to(w.dev).eval()
    torch.save(w.up.state_dict(), w.tmp / "upper.pth")
    torch.save(w.lo.state_dict(), w.tmp / "lower.pth")
    w.runs = {}

    def dense_run(metrics, breakdown):
        key = ("dense", metrics, breakdown)
        if key not in w.runs:
            w.runs[key] = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, 3, batch_size=4, metrics=metrics, breakdown=breakdown)
        return w.runs[key]

    def plain_run(metrics, breakdown, batch_size=1):
        key = ("plain", metrics, breakdown, batch_size)
        if key not in w.runs:
            w.runs[key] = processors.evaluate_full(w.base, None, w.up, w.lo, w.ds, batch_size, False, metrics=metrics, breakdown=breakdown)
        return w.runs[key]

    w.dense_run, w.plain_run = dense_run, plain_run
    return w


def _figures(up, lo, tgt, full):
    """float64 figures of rows [n, 15, 3], [n, 8, 3] against targets [n, 21, 3]: the group figures' names -> values."""
    allj, upper, lower, _ = dense_ref.errors_cm(up, lo, tgt)
    pred = dense_ref.assemble(up, lo)
    tgt = np.asarray(tgt, dtype=np.float64).reshape(-1, 21, 3)
    out = dict(all_cm=allj, upper_cm=upper, lower_cm=lower, rot_deg=float(ref.bone_angles_deg(pred, tgt).mean()))
    if full:
        out.update(pa_cm=float(pm.fit_errors(pred, tgt)[1].mean()) * 100, root_rel_cm=float(pm.root_relative(pred, tgt).mean()) * 100)
    return out


def _check_groups(s, up, lo, tgt, row_rec, full, bins):
    """by_action, by_recording and the percentiles of summary ``s`` against float64 from the counted rows' predictions (row_rec >= 0)."""
    a, r = s["by_action"], s["by_recording"]
    assert a["action"] == list(ACTIONS) and r["recording"] == [0, 1, 2, 3] and r["action"] == list(REC_ACTION) and r["snippet"] == list(REC_SNIPPET)
    names = ("all_cm", "upper_cm", "lower_cm", "rot_deg") + (("pa_cm", "root_rel_cm") if full else ())
    assert set(a) == {"action", "frames", "recordings", "p50_cm", "p90_cm"} | set(names)
    assert set(r) == {"recording", "action", "snippet", "frames", "all_cm"}
    row_act = np.where(row_rec >= 0, np.asarray(REC_ACTION)[np.maximum(row_rec, 0)], -1)
    err_cm = np.linalg.norm(dense_ref.assemble(up, lo) - np.asarray(tgt, dtype=np.float64).reshape(-1, 21, 3), axis=2) * 100       # [rows, 21]
    width = bins[0]
    worst = 0.0
    for i, act in enumerate(ACTIONS):
        m = row_act == act
        assert a["frames"][i] == int(m.sum()) and a["recordings"][i] == len(set(row_rec[m].tolist()))
        if not m.any():
            assert all(a[k][i] is None for k in names + ("p50_cm", "p90_cm")), "an action without a counted frame carries None"
            continue
        want = _figures(up[m], lo[m], tgt[m], full)
        for k in names:
            worst = max(worst, abs(a[k][i] - want[k]))
            assert abs(a[k][i] - want[k]) <= 1e-3, (act, k, a[k][i], want[k])
        for k, q in (("p50_cm", 0.5), ("p90_cm", 0.9)):
            assert abs(a[k][i] - ref.order_statistic(err_cm[m], q)) <= 2 * width, (act, k)
    for rec in range(4):
        m = row_rec == rec
        assert r["frames"][rec] == int(m.sum())
        if not m.any():
            assert r["all_cm"][rec] is None
        else:
            assert abs(r["all_cm"][rec] - float(err_cm[m].mean())) <= 1e-3, rec
    print("group figures: worst difference %.2e (cm, deg)" % worst)
    # the uncovered action: listed, with 0 frames and None figures
    assert a["frames"][2] == 0 and a["recordings"][2] == 0 and a["all_cm"][2] is None and r["frames"][3] == 0
    # percentiles, per-joint medians, PCK AUC
    counted = err_cm[row_rec >= 0]
    p99 = ref.order_statistic(counted, 0.99)
    assert p99 < (bins[1] - 1) * width, "the test's bins hold the float64 p99 below the overflow bin"
    assert s["breakdown"] == bins and s["percentile_clipped"] is False and set(s["percentiles_cm"]) == {50, 90, 95, 99}
    for q, v in s["percentiles_cm"].items():
        print("p%d %.4f cm, order statistic %.4f cm" % (q, v, ref.order_statistic(counted, q / 100.0)))
        assert abs(v - ref.order_statistic(counted, q / 100.0)) <= 2 * width, q
    assert s["per_joint_median_cm"].shape == (21,)
    for j in range(21):
        assert abs(s["per_joint_median_cm"][j] - ref.order_statistic(counted[:, j], 0.5)) <= 2 * width, j
    assert s["joint_errors"] == counted.size == int(s["error_hist"].sum()) and s["dropped"] == 0 and s["beyond"] == int(s["error_hist"][-1])
    assert s["error_hist"].shape == (bins[1],) and s["pck_auc"] == ref.pck_auc(s["error_hist"], width)
    assert abs(s["pck_auc"] - np.mean([(counted < k * width).mean() for k in range(1, 31)])) <= 0.02      # (the curve itself, loosely)


@pytest.mark.parametrize("metrics", ["reference", "full"])
def test_dense_group_figures_against_float64(world, metrics):
    s, a = world.dense_run(metrics, BINS)
    cov = a["covered"] > 0
    assert a["action"].dtype == np.int64 and np.array_equal(a["action"], np.repeat(REC_ACTION, LENGTHS))
    assert cov.sum() == F - 7 and not cov[a["action"] == 5].any()
    row_rec = np.where(cov, a["recording"], -1)
    _check_groups(s, a["upper"], a["lower"], a["target"], row_rec, metrics == "full", BINS)
    # the frames-weighted recombination of the action figures is the pass's own figure
    n = np.asarray(s["by_action"]["frames"], dtype=np.float64)
    for k in ("all_cm", "upper_cm", "lower_cm", "rot_deg") + (("pa_cm", "root_rel_cm") if metrics == "full" else ()):
        v = np.asarray([0.0 if x is None else x for x in s["by_action"][k]])
        assert abs((n * v).sum() / n.sum() - s[k]) <= 1e-3, k
    n = np.asarray(s["by_recording"]["frames"], dtype=np.float64)
    v = np.asarray([0.0 if x is None else x for x in s["by_recording"]["all_cm"]])
    assert abs((n * v).sum() / n.sum() - s["all_cm"]) <= 1e-3


def _window_rows(world, batch_size):
    """The window predictions of an identical pass without the option: the nets over the split's minibatches as _epoch_eval runs them."""
    from mmego_amd.data import DeviceArrays, batch_indices
    from mmego_amd.train_step import call_upper
    arrays, dev = DeviceArrays.of(world.ds, world.dev), world.dev
    ups, los, tgts, recs = [], [], [], []
    with torch.no_grad():
        for idx in batch_indices(len(world.ds), batch_size, False):
            b = arrays.gather(idx)
            B = len(idx)
            h0, c0 = torch.zeros((6, B, 64), device=dev), torch.zeros((6, B, 64), device=dev)
            R, t = world.base.head_pose(None, b["imu"], b["R_R0R"], b["target"])
            up = call_upper(world.up, b["data"], h0, c0, b["skl"], R, t)[0]
            lo, _ = world.lo(up.clone(), b["data"], h0, h0, h0, h0, b["skl"], R, t)
            ups.append(up.reshape(B * T, 15, 3).cpu().numpy())
            los.append(lo.reshape(B * T, 8, 3).cpu().numpy())
            tgts.append(b["target"].reshape(B * T, 21, 3).cpu().numpy())
            recs.append(np.repeat(world.ds.win_rec_[idx], T))
    return np.concatenate(ups), np.concatenate(los), np.concatenate(tgts), np.concatenate(recs)


@pytest.mark.parametrize("metrics,batch_size", [("reference", 1), ("full", 1), ("reference", 3)])
def test_plain_group_figures_against_float64(world, metrics, batch_size):
    _, s = world.plain_run(metrics, BINS, batch_size)
    up, lo, tgt, row_rec = _window_rows(world, batch_size)
    assert len(row_rec) == 4 * T and set(row_rec.tolist()) == {0, 1, 2}
    _check_groups(s, up, lo, tgt, row_rec, metrics == "full", BINS)
    if batch_size == 1:                                    # minibatches of one size: means of minibatch means are plain means
        n = np.asarray(s["by_action"]["frames"], dtype=np.float64)
        for k in ("all_cm", "upper_cm", "lower_cm"):
            v = np.asarray([0.0 if x is None else x for x in s["by_action"][k]])
            assert abs((n * v).sum() / n.sum() - s[k]) <= 1e-3, k


def _same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    return a == b or (a is None and b is None)


@pytest.mark.parametrize("metrics", ["reference", "full"])
def test_no_effect_when_off(world, metrics):
    s0, a0 = world.dense_run(metrics, None)
    s1, a1 = world.dense_run(metrics, BINS)
    assert not (set(s0) & NEW_KEYS) and set(s1) - set(s0) == NEW_KEYS and "action" not in a0
    for k in s0:
        assert _same(s0[k], s1[k]), k
    assert a0["pred"].tobytes() == a1["pred"].tobytes() and set(a1) - set(a0) == {"action"}
    (out0, p0), (out1, p1) = world.plain_run(metrics, None), world.plain_run(metrics, BINS)
    assert not (set(p0) & NEW_KEYS) and set(p1) - set(p0) == NEW_KEYS
    for k in p0:
        assert _same(p0[k], p1[k]), k
    for x, y in zip(out0, out1):
        assert _same(np.asarray(x), np.asarray(y))


def test_the_argument_is_checked_before_anything_runs(world):
    from mmego_amd import dense, processors
    from mmego_amd.data import ArraySplit
    for bad in ((0.3, 64), (0.5, 1), (0.5, 4097), (0.0, 64), 0.5):
        with pytest.raises(ValueError, match="breakdown"):
            dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, breakdown=bad)
        with pytest.raises(ValueError, match="breakdown"):
            processors.evaluate_full(world.base, None, world.up, world.lo, world.ds, 1, False, breakdown=bad)
    z = np.zeros((2, 1), dtype=np.float32)
    with pytest.raises(ValueError, match="breakdown"):
        processors.evaluate_full(world.base, None, world.up, world.lo, ArraySplit(z, z, z, z, z), 1, False, breakdown=BINS)


def test_command_line_prints_the_breakdown_behind_everything_else(world):
    """One `main.py --infer --dense --breakdown --gt_head_pose --save_pred` child, under a time limit of its own."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    path = str(world.tmp / "pred.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--infer", "--dense", "--breakdown", "--gt_head_pose", "--save_pred", path,
                        "--stride", "5", "--data_root", world.data, "--device", "cuda:0", "--seed", "3", "--batch_size", "4",
                        "--load_Upper_path", str(world.tmp / "upper.pth"), "--load_Lower_path", str(world.tmp / "lower.pth")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    out = r.stdout
    lines = ["Average Joint Localization Error(cm):", "Per Joint Localization Error(cm):", "Single-window (unblended) Error(cm):",
             "Window Disagreement(cm):", "Dense windows: ", "Per-frame skeletons saved in", "Joint Error Percentiles(cm): p50 ", "PCK AUC(0-15cm): ",
             "Per Joint Median Error(cm): [", "Action 1 (", "Action 2 (", "Action 5 (0 frames, 0 recordings): all None", "Worst Recordings(cm): action "]
    at = [out.index(line) for line in lines]
    assert at == sorted(at), "the lines come in this order"
    assert len(re.findall(r"^Action \d+ \(", out, flags=re.M)) == 3
    m = re.search(r"^Joint Error Percentiles\(cm\): p50 (%s) p90 (%s) p95 (%s) p99 (%s) \(bins of 0.05 cm; (\d+) of (\d+) joint errors beyond 204.75 cm\)$"
                  % ((NUMBER,) * 4), out, flags=re.M)
    assert m and int(m.group(6)) == (F - 7) * 21 and 0 <= int(m.group(5)) <= int(m.group(6)), out[-3000:]
    assert re.search(r"^Action 2 \(61 frames, 2 recordings\): all %s upper %s lower %s rotation\(°\) %s p50 %s p90 %s$" % ((NUMBER,) * 6), out, flags=re.M)
    worst = re.search(r"^Worst Recordings\(cm\): (.*)$", out, flags=re.M).group(1).split("; ")
    assert len(worst) == 3 and all(re.fullmatch(r"action \d+ snippet \d+: %s \(\d+ frames\)" % NUMBER, w) for w in worst), worst
    z = np.load(path)
    assert {"action", "by_recording_all_cm", "error_hist", "error_hist_bin_cm", "by_action_action", "by_action_frames", "by_action_all_cm"} <= set(z.files)
    assert z["action"].shape == (F,) and z["action"].dtype == np.int64 and np.array_equal(z["action"], np.repeat(REC_ACTION, LENGTHS))
    assert z["by_recording_all_cm"].shape == (4,) and np.isnan(z["by_recording_all_cm"][3]) and np.isfinite(z["by_recording_all_cm"][:3]).all()
    assert z["error_hist"].shape == (4096,) and int(z["error_hist"].sum()) == (F - 7) * 21 and float(z["error_hist_bin_cm"]) == 0.05
    assert z["by_action_action"].tolist() == list(ACTIONS) and z["by_action_frames"].tolist() == [23, 61, 0] and np.isnan(z["by_action_all_cm"][2])
    cov = z["covered"] > 0
    for i, act in enumerate(ACTIONS[:2]):
        m = cov & (z["action"] == act)
        want = np.linalg.norm(z["pred"][m].astype(np.float64) - z["target"][m], axis=2).mean() * 100
        assert abs(z["by_action_all_cm"][i] - want) <= 1e-3, act
