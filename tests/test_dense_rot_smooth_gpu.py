"""GPU: dense inference with the temporal filter of the blended rotations (dense.dense_infer(blend_space="rot", rot_smooth=(H, order,
taper)), `main.py --infer --dense --blend_space rot --rot_smooth H`) on the synthetic Sample_data tree of tests/test_dense_rot_gpu.py:
recordings of 23, 20, 7 and 41 frames (frame_no = 20), stride 3, batch_size 4, nets from torch.manual_seed, the recorded head pose.

What is compared with what: the filtered frames and quaternions with the float64 restatement of tests/rot_smooth_ref.py applied to the
DOWNLOADED blended frames and quaternions, recording by recording (2e-5 m, the project's joint bar; quaternions, moved and rot_moved by
|out - ref| <= 2^-23 |ref| + 1e-7); the blended frames, quaternions and their figures with the plain "rot" pass (bits); every covered
frame's 20 bones with |body_b| (2e-6 m); the saved file's pred with numpy forward kinematics of its rot over its bone_vectors from
pred's roots (2e-5 m); the summary figures with float64 recomputations from the arrays (1e-3 cm; 1e-5 degrees + 2^-22 relative, as
tests/test_dense_rot_gpu.py holds rot_spread_deg)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bone_blend_ref as bref
import dense_ref as ref
import rot_blend_ref as rref
import rot_smooth_ref as rsref
import smooth_ref as sref
from conftest import ROOT
from test_dense_rot_gpu import BONES_ALL, LENGTHS, _make_dataset
from test_dense_smooth_gpu import _same
from test_floor_gpu import _figures, _hold

pytestmark = pytest.mark.gpu

T = 20
F = sum(LENGTHS)
ROT_SMOOTH = (2, 2, "gauss")
NEW_SUMMARY = {"unsmoothed_all_cm", "unsmoothed_upper_cm", "unsmoothed_lower_cm", "unsmoothed_rot_deg", "unsmoothed_per_joint_cm", "moved_cm",
               "rot_moved_deg", "rot_smooth", "rot_smooth_fallback", "rot_jitter_deg", "unsmoothed_rot_jitter_deg"}
NEW_ARRAYS = {"pred_unsmoothed", "rot_unsmoothed", "moved", "rot_moved"}


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
    w.tmp = tmp_path_factory.mktemp("dense_rot_smooth")
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
    w.body = np.asarray(w.ds.frame_bones_, dtype=np.float32).reshape(-1, 3)[:20].copy()
    w.L = np.linalg.norm(w.body.astype(np.float64), axis=1)
    w.runs = {}

    def run(metrics="reference", **more):
        key = (metrics, tuple(sorted(more.items())))
        if key not in w.runs:
            w.runs[key] = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, 3, batch_size=4, metrics=metrics, blend_space="rot", **more)
        return w.runs[key]

    w.run = run
    return w


def _seg(a):
    return np.where(a["covered"] > 0, a["recording"], -1).astype(np.int32)


def _jitter(rot, a):
    """rot_jitter_deg by plain loops and by rotation MATRICES (the pass works in quaternion algebra): frames whose two neighbours are
    covered frames of the same recording, every bone, the quaternions normalised first."""
    tot, n = 0.0, 0
    for f in range(1, F - 1):
        if not (a["covered"][f - 1] and a["covered"][f] and a["covered"][f + 1]) or len({int(a["recording"][g]) for g in (f - 1, f, f + 1)}) != 1:
            continue
        for b in range(20):
            Q0, Q1, Q2 = (rref.matrix(rot[g, b].astype(np.float64) / np.linalg.norm(rot[g, b].astype(np.float64))) for g in (f - 1, f, f + 1))
            tot, n = tot + rref.angle((Q0.T @ Q1).T @ (Q1.T @ Q2)), n + 1
    return float(np.degrees(tot / n))


def test_rot_smooth_none_is_the_call_without_the_argument(world):
    s0, a0 = world.run("full")
    s1, a1 = world.run("full", rot_smooth=None)
    _same(s0, s1)
    _same(a0, a1)
    assert not any("smooth" in k or "jitter" in k or "moved" in k for k in list(s1) + list(a1))


def test_filtered_frames_against_the_restatement(world):
    from mmego_amd import dense
    s0, a0 = world.run("full")
    s, a = world.run("full", rot_smooth=ROT_SMOOTH)
    cov = a["covered"] > 0
    assert cov.sum() == F - 7 and np.array_equal(a["covered"], a0["covered"])
    # the blended frames, their quaternions and their figures are the pass's without the filter
    assert a["pred_unsmoothed"].tobytes() == a0["pred"].tobytes() and a["pred_unsmoothed"].dtype == np.float32
    assert a["rot_unsmoothed"].tobytes() == a0["rot"].tobytes() and a["rot_unsmoothed"].dtype == np.float32
    for k in ("all_cm", "upper_cm", "lower_cm", "rot_deg", "accel_cm"):
        assert s["unsmoothed_" + k] == s0[k] and type(s["unsmoothed_" + k]) is type(s0[k]), k
    assert s["unsmoothed_per_joint_cm"].tobytes() == s0["per_joint_cm"].tobytes()
    for k in ("single_all_cm", "single_upper_cm", "single_lower_cm", "single_rot_deg", "single_bone_dev_cm", "spread_cm", "rot_spread_deg",
              "windows", "covered_frames", "degenerate_bones", "max_cover"):
        assert s[k] == s0[k], k
    assert s["position_cm"].tobytes() == s0["position_cm"].tobytes()
    for k in ("spread", "rot_spread", "bone_vectors", "fallback", "target", "covered"):
        assert a[k].tobytes() == a0[k].tobytes(), k
    for k in ("win_up", "win_lo", "win_q_up", "win_q_lo", "win_R"):
        assert torch.equal(a[k], a0[k]), k
    assert set(s) - set(s0) == NEW_SUMMARY | {"unsmoothed_accel_cm"} and set(s0) <= set(s)
    assert set(a) - set(a0) == NEW_ARRAYS and set(a0) <= set(a)
    assert s["rot_smooth"] == ROT_SMOOTH and s["rot_smooth_fallback"] == 0 and "smooth" not in s and "smooth_fallback" not in s
    sr, ar = world.run("reference", rot_smooth=ROT_SMOOTH)
    assert set(sr) - set(world.run("reference")[0]) == NEW_SUMMARY
    # the filtered frames: the restatement on the blended ones, recording by recording
    seg, w = _seg(a), sref.weights(ROT_SMOOTH[0], ROT_SMOOTH[2])
    assert np.array_equal(w, dense.smooth_weights(ROT_SMOOTH[0], ROT_SMOOTH[2]))
    q0 = np.where(np.isnan(a0["rot"]), 0.0, a0["rot"])             # (uncovered: the blend's zero quaternions; never a tap)
    gaps = []
    up64, qu64, moved64, rmoved64, fb_up = rsref.smooth_rot(a0["upper"].reshape(F, 45), q0[:, :14], seg, w, ROT_SMOOTH[1], bref.UPPER_WALK,
                                                            world.body[:14], min_gap=gaps)
    lo64, ql64, _, _, fb_lo = rsref.smooth_rot(a0["lower"].reshape(F, 24), q0[:, 14:], seg, w, ROT_SMOOTH[1], bref.LOWER_WALK, world.body[14:],
                                               min_gap=gaps)
    assert min(gaps) >= 1e-3 and not fb_up.any() and not fb_lo.any()
    diff = np.abs(a["pred"][cov].astype(np.float64) - ref.assemble(up64, lo64)[cov]).max()
    worst_q = ref.within(a["rot"][cov], np.concatenate([qu64, ql64], axis=1)[cov])
    worst_m, worst_r = ref.within(a["moved"], moved64), ref.within(a["rot_moved"], rmoved64)
    print("pred differs from the restatement by at most %.3e m; worst error / bound quat %.3f moved %.3f rot_moved %.3f; least gap / sum |c| "
          "%.3f; moved_cm %.4f rot_moved_deg %.4f" % (diff, worst_q, worst_m, worst_r, min(gaps), s["moved_cm"], s["rot_moved_deg"]))
    assert diff <= 2e-5 and worst_q <= 1.0 and worst_m <= 1.0 and worst_r <= 1.0
    assert np.abs(a["pred"][cov].astype(np.float64) - a0["pred"][cov]).max() > 1e-4, "the filter moved something"
    assert np.abs(a["rot"][cov].astype(np.float64) - a0["rot"][cov]).max() > 1e-4 and s["moved_cm"] > 0.0 and s["rot_moved_deg"] > 0.0
    # the figures, in float64 from the arrays
    want_moved, want_turn = moved64[cov].mean() * 100, float(np.degrees(rmoved64[cov]).mean())
    want_j, want_j0 = _jitter(a["rot"], a), _jitter(a["rot_unsmoothed"], a)
    print("moved %.6f / %.6f cm  turn %.6f / %.6f deg  jitter %.6f / %.6f deg filtered, %.6f / %.6f blended" % (
        s["moved_cm"], want_moved, s["rot_moved_deg"], want_turn, s["rot_jitter_deg"], want_j, s["unsmoothed_rot_jitter_deg"], want_j0))
    assert abs(s["moved_cm"] - want_moved) <= 1e-3
    for got, want in ((s["rot_moved_deg"], want_turn), (s["rot_jitter_deg"], want_j), (s["unsmoothed_rot_jitter_deg"], want_j0)):
        assert abs(got - want) <= 2.0 ** -22 * want + 1e-5
    assert abs(s["moved_cm"] - a["moved"][cov].astype(np.float64).mean() * 100) <= 1e-3
    assert abs(s["rot_moved_deg"] - np.degrees(a["rot_moved"][cov].astype(np.float64)).mean()) <= 2.0 ** -22 * want_turn + 1e-5
    assert s["rot_jitter_deg"] < s["unsmoothed_rot_jitter_deg"], "the filtered rotations are the smoother ones"
    allj = np.linalg.norm(a["pred"][cov].astype(np.float64) - a["target"][cov], axis=2).mean() * 100
    assert abs(s["all_cm"] - allj) <= 1e-3
    num = den = 0.0
    for r in (0, 1, 3):
        m = a["recording"] == r
        d = a["pred"][m].astype(np.float64) - a["target"][m]
        acc = np.linalg.norm(d[:-2] - 2 * d[1:-1] + d[2:], axis=2)
        num, den = num + acc.mean(axis=1).sum(), den + len(acc)
    print("acceleration error %.4f cm/frame^2 filtered, %.4f blended" % (s["accel_cm"], s["unsmoothed_accel_cm"]))
    assert abs(s["accel_cm"] - num / den * 100) <= 1e-3
    # rigid frames: all 20 bones at rest length; unit quaternions; the uncovered recording stays NaN / zeros
    assert np.abs(a["upper"]).max() < 8.0 and np.abs(a["lower"]).max() < 8.0
    d = np.abs(np.concatenate([bref.bone_lengths(a["upper"][cov].reshape(-1, 45), bref.UPPER_WALK),
                               bref.bone_lengths(a["lower"][cov].reshape(-1, 24), bref.LOWER_WALK)], axis=1) - world.L)
    print("worst | |bone| - L | over %d covered frames: %.3e m; bone_dev_cm %.3e" % (cov.sum(), d.max(), s["bone_dev_cm"]))
    assert d.shape[1] == 20 and d.max() <= 2e-6 and s["bone_dev_cm"] <= 2e-4
    assert np.abs(np.linalg.norm(a["rot"][cov].astype(np.float64), axis=2) - 1.0).max() <= 2e-7
    short = a["recording"] == 2
    assert short.sum() == 7 and not cov[short].any() and cov[~short].all()
    assert np.isnan(a["pred"][short]).all() and np.isnan(a["rot"][short]).all() and np.isnan(a["rot_unsmoothed"][short]).all()
    assert np.isnan(a["pred_unsmoothed"][short]).all() and not np.isnan(a["pred"][~short]).any() and not np.isnan(a["rot"][~short]).any()
    assert not a["upper"][short].any() and not a["lower"][short].any() and not a["moved"][short].any() and not a["rot_moved"][short].any()


def _run(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_command_line_writes_filtered_rotations_that_reproduce_pred(world):
    """`main.py --infer --dense --stride 3 --blend_space rot --rot_smooth 2 --save_pred ...` in a fresh child process: the new lines once
    each, the file's keys, the in-process pass's bits, and from the file ALONE -- pred's roots, rot, bone_vectors -- numpy forward
    kinematics gives pred again."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    path = str(world.tmp / "pred_rot_smooth.npz")
    out = _run(["--infer", "--dense", "--stride", "3", "--gt_head_pose", "--data_root", world.data, "--device", "cuda:0", "--seed", "3",
                "--batch_size", "4", "--load_Upper_path", str(world.tmp / "upper.pth"), "--load_Lower_path", str(world.tmp / "lower.pth"),
                "--blend_space", "rot", "--rot_smooth", "2", "--save_pred", path], env)
    s, a = world.run("reference", rot_smooth=ROT_SMOOTH)
    lines = ["Average Joint Localization Error(cm):", "Window Rotational Disagreement(°): ", "Dense windows:", "Per-frame skeletons saved in",
             "Unsmoothed (blended) Error(cm): all ", "Rotation Smoothing: displacement(cm) ", "Rotational Jitter(°/frame^2): "]
    at = [out.index(line) for line in lines]
    assert at == sorted(at) and all(out.count(line) == 1 for line in lines), "the lines come once each, in this order"
    assert "Unsmoothed Acceleration Error" not in out and "Smoothing Displacement(cm)" not in out
    assert "Rotation Smoothing: displacement(cm) {} mean turn(°) {} (window +-2 frames, order 2, gauss; degenerate bones 0)\n".format(
        s["moved_cm"], s["rot_moved_deg"]) in out
    assert "Rotational Jitter(°/frame^2): {} (blended {})\n".format(s["rot_jitter_deg"], s["unsmoothed_rot_jitter_deg"]) in out
    z = np.load(path)
    plain = {"pred", "covered", "spread", "recording", "frame_in_recording", "target", "stride", "blend", "frame_no", "blend_space",
             "degenerate_bones", "rot", "rot_spread", "bone_vectors"}
    assert set(z.files) == plain | {"pred_unsmoothed", "rot_unsmoothed", "moved", "rot_moved", "rot_smooth_window", "rot_smooth_order",
                                    "rot_smooth_taper"}
    assert int(z["rot_smooth_window"]) == 2 and int(z["rot_smooth_order"]) == 2 and str(z["rot_smooth_taper"]) == "gauss"
    assert str(z["blend_space"]) == "rot" and int(z["degenerate_bones"]) == 0
    for k in ("pred", "rot", "pred_unsmoothed", "rot_unsmoothed", "moved", "rot_moved", "rot_spread", "bone_vectors"):
        assert z[k].tobytes() == a[k].tobytes() and z[k].dtype == a[k].dtype and z[k].shape == a[k].shape, k
    assert z["rot_unsmoothed"].shape == (F, 20, 4) and z["pred_unsmoothed"].shape == (F, 21, 3) and z["moved"].shape == z["rot_moved"].shape == (F,)
    cov = z["covered"] > 0
    assert cov.sum() == F - 7 and np.isnan(z["rot"][~cov]).all() and not np.isnan(z["rot"][cov]).any()
    # forward kinematics from the file alone, in the 21-joint numbering, as tests/test_dense_rot_gpu.py walks it: the upper tree hangs
    # from the head (20), the legs from the hips as the LOWER net placed them (pred's joints 12 and 16)
    pred, rot, body = z["pred"][cov].astype(np.float64), z["rot"][cov].astype(np.float64), z["bone_vectors"].astype(np.float64)
    pos = np.full_like(pred, np.nan)
    pos[:, 20], pos[:, 12], pos[:, 16] = pred[:, 20], pred[:, 12], pred[:, 16]
    for i in range(len(pred)):
        for b, (p, c) in enumerate(BONES_ALL):
            x = pos[i, p] + rref.matrix(rot[i, b]) @ body[b]
            if c in (12, 16) and b < 14:
                continue                                   # (the upper net's hips: overwritten by the lower net's in pred)
            pos[i, c] = x
    worst = np.abs(pos - pred).max()
    print("FK of the saved filtered rotations over the saved rest bones against the saved pred: worst %.3e m over %d frames" % (worst, len(pred)))
    assert not np.isnan(pos).any() and worst <= 2e-5


def test_rot_smooth_goes_with_rot_and_floor_measure_only(world):
    from mmego_amd import dense
    for space in ("joints", "bones", None):
        more = {} if space is None else dict(blend_space=space)
        with pytest.raises(ValueError, match="rot_smooth"):
            dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, rot_smooth=ROT_SMOOTH, **more)
    with pytest.raises(ValueError, match="floor: the clamp"):
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, blend_space="rot", rot_smooth=ROT_SMOOTH, floor=("clamp", 6, 0))
    with pytest.raises(ValueError, match="would not be filtered"):
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, blend_space="rot", rot_smooth=ROT_SMOOTH, smooth=ROT_SMOOTH)
    for bad in ((0, 2, "gauss"), (32, 2, "gauss"), (2, 3, "gauss"), (2, 2, "hann"), (2, 2)):
        with pytest.raises(ValueError, match="rot_smooth"):
            dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, blend_space="rot", rot_smooth=bad)
    # "measure" runs, on the filtered frames
    s0, a0 = world.run("reference", rot_smooth=ROT_SMOOTH)
    s, a = world.run("reference", rot_smooth=ROT_SMOOTH, floor=("measure", 6, 0))
    cov = a["covered"] > 0
    assert a["pred"].tobytes() == a0["pred"].tobytes() and a["rot"].tobytes() == a0["rot"].tobytes() and s["floor"] == ("measure", 6.0, 0.0)
    for k, v in s0.items():
        assert np.array_equal(v, s[k]) if isinstance(v, np.ndarray) else v == s[k], k
    assert set(a) - set(a0) == {"foot_height", "ground", "foot_contact"}
    want, hp = _figures(a["lower"][cov][:, [3, 7]], a["target"][cov][:, [15, 19]], a["ground"][cov], a["foot_contact"][cov], 0.06)
    _hold(s, want)
    assert np.array_equal(a["foot_height"][cov], hp.astype(np.float32)) and np.isnan(a["foot_height"][~cov]).all()
    plain = world.run("reference", floor=("measure", 6, 0))[0]
    assert plain["foot_height_err_cm"] != s["foot_height_err_cm"], "the figures are the filtered frames', not the blended ones'"
