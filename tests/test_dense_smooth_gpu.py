"""GPU: dense inference with its temporal filter (dense.dense_infer(smooth=(H, order, taper)), `main.py --infer --dense --smooth H`)
on the synthetic Sample_data tree of tests/test_dense_infer_gpu.py: recordings of 23, 20, 7 and 41 frames (frame_no = 20), nets from
torch.manual_seed, the recorded head pose.

What is compared with what: smooth=None with the call without the argument (keys and bits); the blended frames kept beside the smoothed
ones with the pass without the filter (bits, and its figures exactly: the same launches on the same rows); the smoothed frames with the
float64 restatement of tests/smooth_ref.py applied to the downloaded blended frames, recording by recording (2e-5 m, the project's joint
parity bound; the kernel tests hold the launch itself to 2^-23 |ref| + 1e-7); under blend_space="bones" every covered frame's 20 bones with
L_b (2e-6 m, as tests/test_dense_bones_gpu.py holds the blend to; the printed figure then stays below 2e-4 cm)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bone_blend_ref as bref
import dense_ref as ref
import smooth_ref as sref
from conftest import ROOT
from test_dense_infer_gpu import LENGTHS, F, T, _World, _make_dataset

pytestmark = pytest.mark.gpu

SMOOTH = (2, 2, "gauss")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The tree, its PosePC with the per-frame clouds, seeded nets, and the dense passes the tests share (each computed once)."""
    assert torch.cuda.is_available()
    from mmego_amd import dense, nets, processors
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import PosePC
    w = _World()
    w.tmp = tmp_path_factory.mktemp("dense_smooth")
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
    w.L_up, w.L_lo = dense.bone_lengths(np.asarray(w.ds.frame_bones_, dtype=np.float32).reshape(-1, 3))
    w.runs = {}

    def run(space=None, metrics="reference", **more):
        key = (space, metrics, tuple(sorted(more.items())))
        if key not in w.runs:
            if space is not None:
                more = dict(more, blend_space=space)
            w.runs[key] = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, 3, batch_size=4, metrics=metrics, **more)
        return w.runs[key]

    w.run = run
    return w


def _same(a0, a1):
    assert set(a0) == set(a1)
    for k, v in a0.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == a1[k].tobytes() and v.dtype == a1[k].dtype and v.shape == a1[k].shape, k
        elif isinstance(v, torch.Tensor):
            assert torch.equal(v, a1[k]), k
        elif isinstance(v, dict):
            assert v == a1[k], k
        elif k != "plan":
            assert v == a1[k] and type(v) is type(a1[k]), k


def _seg(a):
    return np.where(a["covered"] > 0, a["recording"], -1).astype(np.int32)


def test_smooth_none_is_the_call_without_the_argument(world):
    s0, a0 = world.run(None, "full")
    s1, a1 = world.run(None, "full", smooth=None)
    _same(s0, s1)
    _same(a0, a1)
    assert not any("smooth" in k or k in ("moved_cm", "moved") for k in list(s1) + list(a1))


@pytest.mark.parametrize("space", [None, "bones"])
def test_smoothed_frames_against_the_restatement(world, space):
    from mmego_amd import dense
    s0, a0 = world.run(space, "full")
    s, a = world.run(space, "full", smooth=SMOOTH)
    cov = a["covered"] > 0
    assert cov.sum() == F - 7 and np.array_equal(a["covered"], a0["covered"])
    # the blended frames and their figures are the pass's without the filter
    assert a["pred_unsmoothed"].tobytes() == a0["pred"].tobytes() and a["pred_unsmoothed"].dtype == np.float32
    for k in ("all_cm", "upper_cm", "lower_cm", "rot_deg", "accel_cm"):
        assert s["unsmoothed_" + k] == s0[k] and type(s["unsmoothed_" + k]) is type(s0[k]), k
    assert s["unsmoothed_per_joint_cm"].tobytes() == s0["per_joint_cm"].tobytes()
    for k in ("single_all_cm", "single_upper_cm", "single_lower_cm", "single_rot_deg", "spread_cm", "windows", "covered_frames"):
        assert s[k] == s0[k], k
    assert a["spread"].tobytes() == a0["spread"].tobytes() and torch.equal(a["win_up"], a0["win_up"])
    assert set(s) - set(s0) == {"unsmoothed_all_cm", "unsmoothed_upper_cm", "unsmoothed_lower_cm", "unsmoothed_rot_deg",
                                "unsmoothed_per_joint_cm", "unsmoothed_accel_cm", "moved_cm", "smooth", "smooth_fallback"}
    assert set(a) - set(a0) == {"pred_unsmoothed", "moved"} and s["smooth"] == SMOOTH and s["smooth_fallback"] == 0
    # the smoothed frames: the restatement on the blended ones, recording by recording
    seg, w = _seg(a), sref.weights(SMOOTH[0], SMOOTH[2])
    assert np.array_equal(w, dense.smooth_weights(SMOOTH[0], SMOOTH[2]))
    if space == "bones":
        up64, moved64, fb_up = sref.smooth_bones(a0["upper"].reshape(F, 45), seg, w, SMOOTH[1], bref.UPPER_WALK, world.L_up)
        lo64, _, fb_lo = sref.smooth_bones(a0["lower"].reshape(F, 24), seg, w, SMOOTH[1], bref.LOWER_WALK, world.L_lo)
        assert not fb_up.any() and not fb_lo.any()
    else:
        up64, moved64 = sref.smooth_frames(a0["upper"].reshape(F, 45), seg, w, SMOOTH[1])
        lo64, _ = sref.smooth_frames(a0["lower"].reshape(F, 24), seg, w, SMOOTH[1])
    diff = np.abs(a["pred"][cov].astype(np.float64) - ref.assemble(up64, lo64)[cov]).max()
    diff_m = np.abs(a["moved"] - moved64).max()
    print("%s: pred differs from the restatement by at most %.3e m, moved by %.3e m; moved_cm %.4f" % (space, diff, diff_m, s["moved_cm"]))
    assert diff <= 2e-5 and diff_m <= 2e-5
    assert np.abs(a["pred"][cov].astype(np.float64) - a0["pred"][cov]).max() > 1e-4, "the filter moved something"
    assert abs(s["moved_cm"] - moved64[cov].mean() * 100) <= 1e-3 and s["moved_cm"] > 0.0
    # uncovered frames take no part and stay as they were
    assert np.isnan(a["pred"][~cov]).all() and not np.isnan(a["pred"][cov]).any() and not a["moved"][~cov].any()
    assert not a["upper"][~cov].any() and not a["lower"][~cov].any()
    # the figures are the smoothed frames', in float64 from pred and target
    allj = np.linalg.norm(a["pred"][cov].astype(np.float64) - a["target"][cov], axis=2).mean() * 100
    assert abs(s["all_cm"] - allj) <= 1e-3
    num = den = 0.0
    for r in (0, 1, 3):
        m = a["recording"] == r
        d = a["pred"][m].astype(np.float64) - a["target"][m]
        acc = np.linalg.norm(d[:-2] - 2 * d[1:-1] + d[2:], axis=2)
        num, den = num + acc.mean(axis=1).sum(), den + len(acc)
    print("%s: acceleration error %.4f cm/frame^2 smoothed, %.4f blended" % (space, s["accel_cm"], s["unsmoothed_accel_cm"]))
    assert abs(s["accel_cm"] - num / den * 100) <= 1e-3


def test_bones_stay_rigid_under_the_filter(world):
    s, a = world.run("bones", "full", smooth=SMOOTH)
    sj, aj = world.run("joints", "reference", smooth=SMOOTH)
    cov = a["covered"] > 0
    assert np.abs(a["upper"]).max() < 8.0 and np.abs(a["lower"]).max() < 8.0
    d = np.concatenate([bref.bone_length_dev(a["upper"][cov].reshape(-1, 45), bref.UPPER_WALK, world.L_up),
                        bref.bone_length_dev(a["lower"][cov].reshape(-1, 24), bref.LOWER_WALK, world.L_lo)], axis=1)
    print("bones: worst | |bone| - L | %.3e m, bone_dev_cm %.3e; joints: bone_dev_cm %.3e" % (d.max(), s["bone_dev_cm"], sj["bone_dev_cm"]))
    assert d.shape[1] == 20 and d.max() <= 2e-6
    assert abs(s["bone_dev_cm"] - d.mean() * 100) <= 1e-3 and s["bone_dev_cm"] <= 2e-4
    assert s["degenerate_bones"] == 0 and s["smooth_fallback"] == 0 and s["blend_space"] == "bones"
    assert sj["smooth_fallback"] == 0 and sj["bone_dev_cm"] >= s["bone_dev_cm"]


def test_a_bad_smooth_argument_is_refused(world):
    from mmego_amd import dense
    for bad in ((0, 2, "gauss"), (32, 2, "gauss"), (2, 3, "gauss"), (2, 2, "hann"), (2, 2)):
        with pytest.raises(ValueError, match="smooth"):
            dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, smooth=bad)


def test_command_line(world):
    """`main.py --infer --dense --stride 3 --smooth 2 --blend_space bones --metrics full --save_pred ...` in a fresh child process: the
    three new lines behind the existing ones, the new arrays and scalars in the file, the in-process pass's skeletons."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    path = str(world.tmp / "pred.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--infer", "--dense", "--stride", "3", "--gt_head_pose", "--data_root",
                        world.data, "--device", "cuda:0", "--seed", "3", "--batch_size", "4", "--load_Upper_path", str(world.tmp / "upper.pth"),
                        "--load_Lower_path", str(world.tmp / "lower.pth"), "--save_pred", path, "--smooth", "2", "--blend_space", "bones",
                        "--metrics", "full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    out = r.stdout
    lines = ["Average Joint Localization Error(cm):", "Single-window (unblended) Error(cm):", "Window Disagreement(cm):",
             "Bone Length Deviation(cm): blended ", "Dense windows:", "Single-window Acceleration Error(cm/frame^2):",
             "Per-frame skeletons saved in", "Unsmoothed (blended) Error(cm): all ", "Smoothing Displacement(cm): ",
             "Unsmoothed Acceleration Error(cm/frame^2): "]
    at = [out.index(line) for line in lines]
    assert at == sorted(at), "the lines come in this order"
    assert "(window +-2 frames, order 2, gauss; degenerate bones 0)" in out
    s, a = world.run("bones", "full", smooth=SMOOTH)
    assert "Smoothing Displacement(cm): {} (".format(s["moved_cm"]) in out
    assert "Unsmoothed Acceleration Error(cm/frame^2): {}\n".format(s["unsmoothed_accel_cm"]) in out
    z = np.load(path)
    today = {"pred", "covered", "spread", "recording", "frame_in_recording", "target", "stride", "blend", "frame_no"}
    assert set(z.files) == today | {"blend_space", "degenerate_bones", "pred_unsmoothed", "moved", "smooth_window", "smooth_order", "smooth_taper"}
    assert int(z["smooth_window"]) == 2 and int(z["smooth_order"]) == 2 and str(z["smooth_taper"]) == "gauss"
    assert z["pred"].tobytes() == a["pred"].tobytes() and z["pred_unsmoothed"].tobytes() == a["pred_unsmoothed"].tobytes()
    assert z["moved"].tobytes() == a["moved"].tobytes() and z["moved"].shape == (F,) and z["pred_unsmoothed"].shape == (F, 21, 3)
