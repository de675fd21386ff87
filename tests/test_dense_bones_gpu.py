"""GPU: dense inference with the bone-length-preserving blend (dense.dense_infer(blend_space="bones"), `main.py --infer --dense
--blend_space bones`) on the synthetic Sample_data tree of tests/test_dense_infer_gpu.py: recordings of 23, 20, 7 and 41 frames
(frame_no = 20), nets from torch.manual_seed, the recorded head pose.

What is compared with what: the blended frames with the float64 restatement of tests/bone_blend_ref.py applied to the downloaded window
rows (|out - ref| <= 2^-23 |ref| + 1e-7); every covered frame's 20 bones with L_b = float32(|body_b|) (2e-6 m: two float-rounded
endpoints at |coordinate| < 8 m, 2 sqrt(3) 2^-24 8 = 1.7e-6; the range is asserted); blend_space="joints" with the call without the
argument (bits); the summary figures with float64 recomputations (1e-3 cm, the project's bar for the error metric)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io as scio
import torch

import bone_blend_ref as bref
import dense_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

T = 20
LENGTHS = (23, 20, 7, 41)
F = sum(LENGTHS)
LINE = "Bone Length Deviation(cm): blended "


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
    w.tmp = tmp_path_factory.mktemp("dense_bones")
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

    def run(blend, space):
        key = (blend, space)
        if key not in w.runs:
            more = {} if space is None else dict(blend_space=space)
            s, a = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, 3, blend=blend, batch_size=4, **more)
            a = dict(a, win_up_h=a["win_up"].cpu().numpy(), win_lo_h=a["win_lo"].cpu().numpy())
            w.runs[key] = (s, a)
        return w.runs[key]

    w.run = run
    return w


def _bone_dev_cm(world, up, lo):
    """The mean over rows and the 20 bones of | |bone| - L_b |, in cm, in float64."""
    d = np.concatenate([bref.bone_length_dev(up, bref.UPPER_WALK, world.L_up), bref.bone_length_dev(lo, bref.LOWER_WALK, world.L_lo)], axis=1)
    assert d.shape[1] == 20
    return float(d.mean()) * 100, d


@pytest.mark.parametrize("blend", ["mean", "triangle"])
def test_stride_3_bones_against_the_restatement(world, blend):
    s, a = world.run(blend, "bones")
    plan = a["plan"]
    assert plan.W == 2 + 1 + 8 and s["covered_frames"] == F - 7 and s["blend_space"] == "bones"
    up64, spr64, fb_up = bref.blend_bones(a["win_up_h"], plan.cov_off, plan.cov_row, plan.cov_w, bref.UPPER_WALK, world.L_up)
    lo64, _, fb_lo = bref.blend_bones(a["win_lo_h"], plan.cov_off, plan.cov_row, plan.cov_w, bref.LOWER_WALK, world.L_lo)
    cov = a["covered"] > 0
    worst_u, worst_l = ref.within(a["upper"].reshape(F, 45), up64), ref.within(a["lower"].reshape(F, 24), lo64)
    worst = ref.within(a["pred"][cov], ref.assemble(up64, lo64)[cov])
    worst_s = ref.within(a["spread"], spr64)
    print("stride 3 %s bones: worst error / bound upper %.3f lower %.3f pred %.3f spread %.3f" % (blend, worst_u, worst_l, worst, worst_s))
    assert worst_u <= 1.0 and worst_l <= 1.0 and worst <= 1.0 and worst_s <= 1.0
    # every covered frame is a rigid skeleton again
    assert np.abs(a["upper"]).max() < 8.0 and np.abs(a["lower"]).max() < 8.0
    _, d = _bone_dev_cm(world, a["upper"][cov].reshape(-1, 45), a["lower"][cov].reshape(-1, 24))
    print("worst | |bone| - L | over %d covered frames: %.3e m" % (cov.sum(), d.max()))
    assert d.max() <= 2e-6
    # the uncovered recording, as before
    short = a["recording"] == 2
    assert short.sum() == 7 and (a["covered"][short] == 0).all() and np.isnan(a["pred"][short]).all() and not np.isnan(a["pred"][~short]).any()
    assert not a["upper"][short].any() and not a["lower"][short].any() and (a["spread"][short] == 0.0).all()
    assert s["degenerate_bones"] == 0 and not a["fallback"].any() and a["fallback"].shape == (F,) and not fb_up.any() and not fb_lo.any()
    # frames covered once carry their window's prediction
    once = np.flatnonzero(a["covered"] == 1)
    rows = plan.cov_row[plan.cov_off[once]]
    assert len(once) and np.array_equal(a["upper"][once].reshape(-1, 45), a["win_up_h"][rows])


def test_joints_is_the_call_without_the_argument(world):
    s0, a0 = world.run("mean", None)
    s1, a1 = world.run("mean", "joints")
    assert set(a1) - set(a0) == {"fallback"} and set(s1) - set(s0) == {"bone_dev_cm", "single_bone_dev_cm", "degenerate_bones", "blend_space"}
    assert set(a0) <= set(a1) and set(s0) <= set(s1)
    for k, v in a0.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == a1[k].tobytes() and v.dtype == a1[k].dtype, k
        elif isinstance(v, torch.Tensor):
            assert torch.equal(v, a1[k]), k
    for k, v in s0.items():
        assert (v.tobytes() == s1[k].tobytes()) if isinstance(v, np.ndarray) else (v == s1[k] and type(v) is type(s1[k])), k
    assert s1["degenerate_bones"] == 0 and not a1["fallback"].any() and s1["blend_space"] == "joints"


@pytest.mark.parametrize("blend", ["mean", "triangle"])
def test_summary_figures(world, blend):
    sb, ab = world.run(blend, "bones")
    sj, aj = world.run(blend, "joints")
    cov = ab["covered"] > 0
    want, _ = _bone_dev_cm(world, ab["upper"][cov].reshape(-1, 45), ab["lower"][cov].reshape(-1, 24))
    single, _ = _bone_dev_cm(world, ab["win_up_h"], ab["win_lo_h"])
    allj = np.linalg.norm(ab["pred"][cov].astype(np.float64) - ab["target"][cov], axis=2).mean() * 100
    _, upper, lower, _ = ref.errors_cm(ab["upper"][cov], ab["lower"][cov], ab["target"][cov])
    print("bones %s: bone_dev %.6f / %.6f  single %.6f / %.6f  all %.6f / %.6f  upper %.6f / %.6f  lower %.6f / %.6f cm" % (
        blend, sb["bone_dev_cm"], want, sb["single_bone_dev_cm"], single, sb["all_cm"], allj, sb["upper_cm"], upper, sb["lower_cm"], lower))
    assert abs(sb["bone_dev_cm"] - want) <= 1e-3 and abs(sb["single_bone_dev_cm"] - single) <= 1e-3
    assert abs(sb["all_cm"] - allj) <= 1e-3 and abs(sb["upper_cm"] - upper) <= 1e-3 and abs(sb["lower_cm"] - lower) <= 1e-3
    # the joints pass: the same figure from its own rows, and never below the rigid pass's (the vector mean can only shorten a bone)
    wantj, _ = _bone_dev_cm(world, aj["upper"][cov].reshape(-1, 45), aj["lower"][cov].reshape(-1, 24))
    print("joints %s: bone_dev %.6f / %.6f cm, single %.6f cm" % (blend, sj["bone_dev_cm"], wantj, sj["single_bone_dev_cm"]))
    assert abs(sj["bone_dev_cm"] - wantj) <= 1e-3 and sj["single_bone_dev_cm"] == sb["single_bone_dev_cm"]
    assert sj["bone_dev_cm"] >= sb["bone_dev_cm"] - 2e-4
    # the single-window figures and the window rows do not depend on the blend space
    assert torch.equal(ab["win_up"], aj["win_up"]) and torch.equal(ab["win_lo"], aj["win_lo"])
    for k in ("single_all_cm", "single_upper_cm", "single_lower_cm", "single_rot_deg"):
        assert sb[k] == sj[k], k


def test_an_unknown_blend_space_is_refused(world):
    from mmego_amd import dense
    with pytest.raises(ValueError, match="blend_space"):
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, blend_space="rotations")


def _run(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_command_line_writes_the_same_rigid_skeletons_twice(world):
    """`main.py --infer --dense --stride 3 --blend_space bones --save_pred ...` twice, each in a fresh child process, and once without
    the flag: the same bytes twice, the new line and the new scalars with the flag only."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    common = ["--infer", "--dense", "--stride", "3", "--gt_head_pose", "--data_root", world.data, "--device", "cuda:0", "--seed", "3",
              "--batch_size", "4", "--load_Upper_path", str(world.tmp / "upper.pth"), "--load_Lower_path", str(world.tmp / "lower.pth")]
    outs, blobs = [], []
    for i, extra in enumerate((["--blend_space", "bones"], ["--blend_space", "bones"], [])):
        path = str(world.tmp / ("pred%d.npz" % i))
        outs.append(_run(common + ["--save_pred", path] + extra, env))
        blobs.append(open(path, "rb").read())
    assert blobs[0] == blobs[1]
    today = {"pred", "covered", "spread", "recording", "frame_in_recording", "target", "stride", "blend", "frame_no"}
    z, plain = np.load(str(world.tmp / "pred0.npz")), np.load(str(world.tmp / "pred2.npz"))
    assert set(z.files) == today | {"blend_space", "degenerate_bones"} and set(plain.files) == today
    assert str(z["blend_space"]) == "bones" and int(z["degenerate_bones"]) == 0 and int(z["stride"]) == 3
    for out in outs[:2]:
        assert out.count(LINE) == 1 and "(degenerate bones 0)" in out
        assert out.index("Window Disagreement(cm):") < out.index(LINE) < out.index("Dense windows:")
    assert "Bone Length Deviation" not in outs[2]
    # the file's skeletons are the in-process pass's, and rigid
    _, a = world.run("mean", "bones")
    assert a["pred"].tobytes() == z["pred"].tobytes()
    assert plain["pred"].tobytes() == world.run("mean", None)[1]["pred"].tobytes()
