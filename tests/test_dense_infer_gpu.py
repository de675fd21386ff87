"""GPU: dense inference (dense.dense_infer, `main.py --infer --dense`) on a tiny synthetic Sample_data tree with the .mat keys of
tests/test_cli_gpu.py but recordings of 23, 20, 7 and 41 frames (frame_no = 20): one with a head window, one that is exactly a window, one
too short for any, one with two reference windows and a frame left over.  Nets from torch.manual_seed, the recorded head pose.

What is compared with what: the stored window rows with the plain path window by window (bits); the blended frames with the float64
restatement of tests/dense_ref.py applied to the downloaded window rows (|out - ref| <= 2^-23 |ref| + 1e-7); the printed error figures
with float64 recomputations (1e-3 cm, the project's bar for the error metric); window minibatches of 1 and 4 with each other (2e-5 m,
the project's joint parity bound: kernels choose forms by size, so no bit equality there)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.io as scio
import torch

import dense_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

T = 20
LENGTHS = (23, 20, 7, 41)
F = sum(LENGTHS)
NUMBER = r"[-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?"


def _make_dataset(root, rng):
    """Action 01: s0 (two frames: the very first snippet, which the loader skips as the reference does) and s1 of 23 frames; action 02:
    s1, s2, s3 of 20, 7 and 41 frames."""
    for a, s, count in ((1, 0, 2), (1, 1, LENGTHS[0]), (2, 1, LENGTHS[1]), (2, 2, LENGTHS[2]), (2, 3, LENGTHS[3])):
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
    """The tree, its PosePC with the per-frame clouds, seeded nets, and the dense passes the tests share (each computed once)."""
    assert torch.cuda.is_available()
    from mmego_amd import dense, nets, processors
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import PosePC
    w = _World()
    w.tmp = tmp_path_factory.mktemp("dense")
    w.data = str(w.tmp / "Sample_data")
    _make_dataset(w.data, np.random.default_rng(0))
    np.random.seed(3)
    w.ds = PosePC(train=False, vis=True, keep_frames=True, batch_length=T, root=w.data)
    assert len(w.ds.frame_npts_) == F and len(w.ds) == 4
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

    def run(stride, blend="mean", batch_size=4, metrics="reference"):
        key = (stride, blend, batch_size, metrics)
        if key not in w.runs:
            s, a = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, stride, blend=blend, batch_size=batch_size, metrics=metrics)
            a = dict(a, win_up_h=a["win_up"].cpu().numpy(), win_lo_h=a["win_lo"].cpu().numpy())
            w.runs[key] = (s, a)
        return w.runs[key]

    w.run = run
    return w


def test_stride_T_is_the_plain_path_window_by_window(world):
    from mmego_amd.train_step import call_upper
    s, a = world.run(T, "mean", 1)
    plan, dev = a["plan"], world.dev
    assert plan.W == 2 + 1 + 0 + 3 and s["windows"] == 6 and s["frames"] == F and s["covered_frames"] == F - 7 and s["max_cover"] == 2
    h0, c0 = torch.zeros((6, 1, 64), device=dev), torch.zeros((6, 1, 64), device=dev)
    with torch.no_grad():
        for w in range(plan.W):
            b = plan.gather([w])
            R, t = world.base.head_pose(None, b["imu"], b["R_R0R"], b["target"])
            up = call_upper(world.up, b["data"], h0, c0, b["skl"], R, t)[0]
            lo, _ = world.lo(up.clone(), b["data"], h0, h0, h0, h0, b["skl"], R, t)
            assert torch.equal(a["win_up"][w * T:(w + 1) * T], up.reshape(T, 45)), w
            assert torch.equal(a["win_lo"][w * T:(w + 1) * T], lo.reshape(T, 24)), w
    # frames covered once carry exactly their window's prediction
    once = np.flatnonzero(a["covered"] == 1)
    assert len(once) == 6 + 20 + 22                   # (23 frames: 3 at either end; 41 frames: windows at 0, 1 and 21)
    rows = plan.cov_row[plan.cov_off[once]]
    want = ref.assemble(a["win_up_h"][rows], a["win_lo_h"][rows]).astype(np.float32)
    assert np.array_equal(a["pred"][once], want)
    assert (a["spread"][once] == 0.0).all() and (a["spread"][a["covered"] == 2] > 0.0).all()
    # the 7-frame recording: no window, no skeleton
    short = a["recording"] == 2
    assert short.sum() == 7 and (a["covered"][short] == 0).all() and np.isnan(a["pred"][short]).all()
    assert not np.isnan(a["pred"][~short]).any() and (a["covered"][~short] >= 1).all()
    assert np.array_equal(a["frame_in_recording"], np.concatenate([np.arange(n) for n in LENGTHS]))
    assert np.array_equal(a["target"], np.asarray(world.ds.frame_key_, dtype=np.float32))


@pytest.mark.parametrize("blend", ["mean", "triangle"])
def test_stride_3_against_the_restatement(world, blend):
    """(upper_cm is recomputed from the blended UPPER rows -- arrays["upper"], checked here to be pred's joints outside the hips --
    because the figure is the Upper net's 15 joints, hips included, while pred carries the Lower net's hips.)"""
    s, a = world.run(3, blend, 4)
    plan = a["plan"]
    assert plan.W == 2 + 1 + 8 and s["covered_frames"] == F - 7 and s["max_cover"] == plan.covered.max() <= 8
    up64, _ = ref.blend(a["win_up_h"], plan.cov_off, plan.cov_row, plan.cov_w)
    lo64, _ = ref.blend(a["win_lo_h"], plan.cov_off, plan.cov_row, plan.cov_w, spread=False)
    _, spr64 = ref.blend(a["win_up_h"], plan.cov_off, plan.cov_row, plan.cov_w)
    cov = a["covered"] > 0
    worst = ref.within(a["pred"][cov], ref.assemble(up64, lo64)[cov])
    worst_s = ref.within(a["spread"], spr64)
    print("stride 3 %s: pred worst error / bound %.3f, spread %.3f" % (blend, worst, worst_s))
    assert worst <= 1.0 and worst_s <= 1.0
    assert np.isnan(a["pred"][~cov]).all() and (a["spread"][~cov] == 0.0).all()
    outside_hips = [j for j in ref.UPPER_MAP if j not in ref.LOWER_MAP]
    assert np.array_equal(a["upper"][:, [ref.UPPER_MAP.index(j) for j in outside_hips]][cov], a["pred"][:, outside_hips][cov])
    assert np.array_equal(a["pred"][:, list(ref.LOWER_MAP)][cov], a["lower"][cov])
    # the figures, in float64 from pred and target
    allj = np.linalg.norm(a["pred"][cov].astype(np.float64) - a["target"][cov], axis=2).mean() * 100
    _, upper, lower, _ = ref.errors_cm(a["upper"][cov], a["lower"][cov], a["target"][cov])
    print("all %.6f / %.6f  upper %.6f / %.6f  lower %.6f / %.6f cm" % (s["all_cm"], allj, s["upper_cm"], upper, s["lower_cm"], lower))
    assert abs(s["all_cm"] - allj) <= 1e-3 and abs(s["upper_cm"] - upper) <= 1e-3 and abs(s["lower_cm"] - lower) <= 1e-3
    assert abs(s["spread_cm"] - spr64[cov].mean() * 100) <= 1e-3
    # by position in the window, from the downloaded window rows
    tgt_rows = a["target"][plan.row_frame]
    sall, sup, slo, per_row = ref.errors_cm(a["win_up_h"], a["win_lo_h"], tgt_rows)
    pos = per_row.reshape(plan.W, T).mean(axis=0)
    print("position_cm worst difference %.2e cm" % np.abs(s["position_cm"] - pos).max())
    assert s["position_cm"].shape == (T,) and np.abs(s["position_cm"] - pos).max() <= 1e-3
    assert abs(s["single_all_cm"] - sall) <= 1e-3 and abs(s["single_upper_cm"] - sup) <= 1e-3 and abs(s["single_lower_cm"] - slo) <= 1e-3


def test_single_figures_on_the_reference_windows_are_evaluate_full(world):
    from mmego_amd import processors
    s, a = world.run(T, "mean", 1)
    plan = a["plan"]
    _, s_ref = processors.evaluate_full(world.base, None, world.up, world.lo, world.ds, 1, False)
    mine = np.flatnonzero(np.isin(plan.starts, world.ds.win_start_))
    assert len(mine) == len(world.ds.win_start_) == 4
    rows = (mine[:, None] * T + np.arange(T)).ravel()
    sall, sup, slo, _ = ref.errors_cm(a["win_up_h"][rows], a["win_lo_h"][rows], a["target"][plan.row_frame[rows]])
    print("all %.6f / %.6f  upper %.6f / %.6f  lower %.6f / %.6f cm" % (s_ref["all_cm"], sall, s_ref["upper_cm"], sup, s_ref["lower_cm"], slo))
    assert abs(s_ref["all_cm"] - sall) <= 1e-3 and abs(s_ref["upper_cm"] - sup) <= 1e-3 and abs(s_ref["lower_cm"] - slo) <= 1e-3


def test_window_minibatch_1_against_4(world):
    _, a1 = world.run(3, "mean", 1)
    _, a4 = world.run(3, "mean", 4)
    cov = a1["covered"] > 0
    diff = np.abs(a1["pred"][cov].astype(np.float64) - a4["pred"][cov]).max()
    print("window minibatch 1 against 4: pred differs by at most %.3e m" % diff)
    assert diff <= 2e-5 and np.array_equal(a1["covered"], a4["covered"])


def test_metrics_full_sees_the_seams(world):
    s, a = world.run(T, "mean", 4, "full")
    for k in ("root_rel_cm", "rigid_cm", "pa_cm", "align_rot_deg", "accel_cm", "single_accel_cm"):
        assert np.isfinite(s[k]), k
    # the blended acceleration error of the three covered recordings, in float64 from pred: second differences ACROSS window seams
    num = den = 0.0
    for r in (0, 1, 3):
        m = a["recording"] == r
        d = a["pred"][m].astype(np.float64) - a["target"][m]
        acc = np.linalg.norm(d[:-2] - 2 * d[1:-1] + d[2:], axis=2)
        num, den = num + acc.mean(axis=1).sum(), den + len(acc)
    assert abs(s["accel_cm"] - num / den * 100) <= 1e-3
    assert world.run(3, "mean", 4, "full")[0]["single_accel_cm"] is None


def _run(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_command_line_writes_the_same_skeletons_twice(world):
    """Two `main.py --infer --dense --stride 5 --blend triangle --save_pred ... --gt_head_pose` runs (the second with --metrics full as
    well: the aligned lines and a finite acceleration error, and figures that leave the skeletons alone)."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    outs, files = [], []
    for i, extra in enumerate(([], ["--metrics", "full"])):
        path = str(world.tmp / ("pred%d.npz" % i))
        outs.append(_run(["--infer", "--dense", "--stride", "5", "--blend", "triangle", "--save_pred", path, "--gt_head_pose", "--data_root",
                          world.data, "--device", "cuda:0", "--seed", "3", "--batch_size", "4", "--load_Upper_path", str(world.tmp / "upper.pth"),
                          "--load_Lower_path", str(world.tmp / "lower.pth")] + extra, env))
        files.append(np.load(path))
    lines = ["Average Joint Localization Error(cm):", "Average UpperBody Joint Localization Error(cm):",
             "Average LowerBody Joint Localization Error(cm):", "Average Joint Rotation Error", "Per Joint Localization Error(cm):",
             "Single-window (unblended) Error(cm):", "Error by window position(cm): [", "Window Disagreement(cm):",
             "Dense windows: 9 windows of 20 frames at stride 5 (blend triangle), 84 of 91 frames covered, largest cover 5"]
    for out in outs:
        at = [out.index(line) for line in lines]
        assert at == sorted(at), "the lines come in this order"
    assert "Joint Error(cm)" not in outs[0] and "PCK@" not in outs[0]
    rest = outs[1][outs[1].index(lines[-1]):]
    for name in ("Root-relative Joint Error(cm)", "Rigid-aligned Joint Error(cm)", "Procrustes-aligned (PA-MPJPE) Joint Error(cm)", "PCK@5cm",
                 "Per Joint Procrustes-aligned Error(cm)"):
        assert name in rest, name
    m = re.search(r"^Acceleration Error\(cm/frame\^2\): (%s)$" % NUMBER, rest, flags=re.M)
    assert m and np.isfinite(float(m.group(1))), rest
    shapes = {"pred": (F, 21, 3), "covered": (F,), "spread": (F,), "recording": (F,), "frame_in_recording": (F,), "target": (F, 21, 3),
              "stride": (), "blend": (), "frame_no": ()}
    for z in files:
        assert set(z.files) == set(shapes)
        for k, shape in shapes.items():
            assert z[k].shape == shape, k
        assert int(z["stride"]) == 5 and str(z["blend"]) == "triangle" and int(z["frame_no"]) == T and z["pred"].dtype == np.float32
        assert np.isnan(z["pred"][z["covered"] == 0]).all() and (z["covered"] == 0).sum() == 7 and not np.isnan(z["pred"][z["covered"] > 0]).any()
    assert files[0]["pred"].tobytes() == files[1]["pred"].tobytes()
    # and they are what the in-process pass gives on the same tree, seed and nets
    _, a = world.run(5, "triangle", 4)
    assert a["pred"].tobytes() == files[0]["pred"].tobytes()
