"""GPU: dense inference with the blend in rotation space (dense.dense_infer(blend_space="rot"), `main.py --infer --dense
--blend_space rot`) on a synthetic Sample_data tree like that of tests/test_dense_bones_gpu.py: recordings of 23, 20, 7 and 41 frames
(frame_no = 20), nets from torch.manual_seed, the recorded head pose -- here with every R_btc a PROPER rotation, as a recording's is
(asserted on the head rotations the rows ran with).

What is compared with what: the blended frames, quaternions and both spreads with the float64 restatement of tests/rot_blend_ref.py
applied to the downloaded window rows (|out - ref| <= 2^-23 |ref| + 1e-7); every covered frame's 20 bones with |body_b| (2e-6 m: two
float-rounded endpoints at |coordinate| < 8 m; the range is asserted); the saved file's pred with numpy forward kinematics of its rot
over its bone_vectors from pred's roots (2e-5 m, the project's joint bar); at stride == frame_no, pred with the "joints" pass (bits);
"joints" and "bones" with themselves (bits); the summary figures with float64 recomputations (1e-3 cm, the project's metric bar)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io as scio
import torch

import bone_blend_ref as bref
import dense_ref as ref
import rot_blend_ref as rref
from conftest import ROOT

pytestmark = pytest.mark.gpu

T = 20
LENGTHS = (23, 20, 7, 41)
F = sum(LENGTHS)
LINE = "Window Rotational Disagreement(°): "
BONES_ALL = ((20, 3), (3, 2), (2, 1), (2, 4), (2, 8), (4, 5), (5, 6), (6, 7), (8, 9), (9, 10), (10, 11), (1, 0), (0, 12), (0, 16),
             (12, 13), (13, 14), (14, 15), (16, 17), (17, 18), (18, 19))          # (parent, child), the 21-joint numbering


def _make_dataset(root, rng):
    """Action 01: s0 (two frames: the very first snippet, which the loader skips as the reference does) and s1 of 23 frames; action 02:
    s1, s2, s3 of 20, 7 and 41 frames.  R_btc: a proper rotation (a column flipped where the determinant is negative)."""
    for a, s, count in ((1, 0, 2), (1, 1, LENGTHS[0]), (2, 1, LENGTHS[1]), (2, 2, LENGTHS[2]), (2, 3, LENGTHS[3])):
        d = os.path.join(root, "%02d" % a, "s%d" % s)
        os.makedirs(d)
        skel = rng.normal(0, 0.4, (32, 3)) + np.array([0.8, 0.0, 0.2])
        for f in range(count):
            n = int(rng.integers(20, 150))
            pc = np.concatenate([rng.normal([0.8, 0.0, 0.2], 0.4, (n, 3)), rng.uniform(10, 46, (n, 1)), rng.normal(0, 0.4, (n, 1))], 1)
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if np.linalg.det(q) < 0:
                q[:, 0] *= -1.0
            assert np.linalg.det(q) > 0.999
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
    w.tmp = tmp_path_factory.mktemp("dense_rot")
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

    def run(blend, space, stride=3, tag=0):
        key = (blend, space, stride, tag)
        if key not in w.runs:
            more = {} if space is None else dict(blend_space=space)
            s, a = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, stride, blend=blend, batch_size=4, **more)
            a = dict(a)
            for k in ("win_up", "win_lo", "win_q_up", "win_q_lo", "win_R"):
                if k in a:
                    a[k + "_h"] = a[k].cpu().numpy()
            w.runs[key] = (s, a)
        return w.runs[key]

    w.run = run
    return w


def _restated(world, a):
    plan = a["plan"]
    cover = (plan.cov_off, plan.cov_row, plan.cov_w)
    gaps = []
    up = rref.blend_rot(a["win_up_h"], a["win_q_up_h"], a["win_R_h"], *cover, rref.UPPER_WALK, rref.ROT_UPPER, world.body[:14], min_gap=gaps)
    lo = rref.blend_rot(a["win_lo_h"], a["win_q_lo_h"], a["win_R_h"], *cover, rref.LOWER_WALK, rref.ROT_LOWER, world.body[14:], min_gap=gaps)
    return up, lo, min(gaps)


@pytest.mark.parametrize("blend", ["mean", "triangle"])
def test_stride_3_rot_against_the_restatement(world, blend):
    s, a = world.run(blend, "rot")
    plan = a["plan"]
    assert plan.W == 2 + 1 + 8 and s["covered_frames"] == F - 7 and s["blend_space"] == "rot"
    assert a["win_q_up_h"].shape == (plan.W * T, 14, 9) and a["win_q_lo_h"].shape == (plan.W * T, 6, 9) and a["win_R_h"].shape == (plan.W * T, 9)
    R = a["win_R_h"].astype(np.float64).reshape(-1, 3, 3)
    assert np.all(np.linalg.det(R) > 0.999) and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5, "the head rotations are proper"
    (up64, qu64, spr64, rspr64, fb_up), (lo64, ql64, _, _, fb_lo), gap = _restated(world, a)
    cov = a["covered"] > 0
    worst_u, worst_l = ref.within(a["upper"].reshape(F, 45), up64), ref.within(a["lower"].reshape(F, 24), lo64)
    worst = ref.within(a["pred"][cov], ref.assemble(up64, lo64)[cov])
    worst_q = ref.within(rref.canonical(a["rot"][cov]), np.concatenate([qu64, ql64], axis=1)[cov])
    worst_s, worst_r = ref.within(a["spread"], spr64), ref.within(a["rot_spread"], rspr64)
    print("stride 3 %s rot: worst error / bound upper %.3f lower %.3f pred %.3f quat %.3f spread %.3f rot_spread %.3f; least gap / W %.3f"
          % (blend, worst_u, worst_l, worst, worst_q, worst_s, worst_r, gap))
    assert gap >= 1e-3, "the restatement's eigenvector is well conditioned on these rows"
    assert worst_u <= 1.0 and worst_l <= 1.0 and worst <= 1.0 and worst_q <= 1.0 and worst_s <= 1.0 and worst_r <= 1.0
    # every covered frame is a rigid skeleton: all 20 bones at their rest lengths
    assert np.abs(a["upper"]).max() < 8.0 and np.abs(a["lower"]).max() < 8.0
    d = np.abs(np.concatenate([bref.bone_lengths(a["upper"][cov].reshape(-1, 45), bref.UPPER_WALK),
                               bref.bone_lengths(a["lower"][cov].reshape(-1, 24), bref.LOWER_WALK)], axis=1) - world.L)
    print("worst | |bone| - L | over %d covered frames: %.3e m" % (cov.sum(), d.max()))
    assert d.shape[1] == 20 and d.max() <= 2e-6
    # the uncovered recording: NaN in the per-frame arrays of the file, zeros in the nets' own rows
    short = a["recording"] == 2
    assert short.sum() == 7 and (a["covered"][short] == 0).all() and np.isnan(a["pred"][short]).all() and not np.isnan(a["pred"][~short]).any()
    assert a["rot"].shape == (F, 20, 4) and a["rot"].dtype == np.float32 and np.isnan(a["rot"][short]).all() and not np.isnan(a["rot"][~short]).any()
    assert not a["upper"][short].any() and (a["spread"][short] == 0.0).all() and (a["rot_spread"][short] == 0.0).all()
    assert s["degenerate_bones"] == 0 and not a["fallback"].any() and not fb_up.any() and not fb_lo.any()
    assert np.abs(np.linalg.norm(a["rot"][cov].astype(np.float64), axis=2) - 1.0).max() <= 2e-7
    assert rspr64[cov & (a["covered"] > 1)].min() > 1e-4, "windows of these random nets do disagree"
    # frames covered once carry their window's prediction
    once = np.flatnonzero(a["covered"] == 1)
    rows = plan.cov_row[plan.cov_off[once]]
    assert len(once) and np.array_equal(a["upper"][once].reshape(-1, 45), a["win_up_h"][rows]) and not a["rot_spread"][once].any()


def test_stride_20_is_the_joints_pass_bit_for_bit(world):
    """stride == frame_no: a frame is covered once -- except where a recording's first window, kept so that its first frames are
    served at all, overlaps the next one (recordings of 23 and 41 frames: 17 + 19 frames covered twice).  Every frame covered once is
    the "joints" pass's frame bit for bit and has no rotational spread; the 20-frame recording is covered once throughout."""
    sr, ar = world.run("mean", "rot", stride=T)
    sj, aj = world.run("mean", "joints", stride=T)
    once = ar["covered"] == 1
    assert once[ar["recording"] == 1].all() and once.sum() == F - 7 - (17 + 19) and set(ar["covered"].tolist()) == {0, 1, 2}
    assert ar["pred"][once].tobytes() == aj["pred"][once].tobytes() and ar["upper"][once].tobytes() == aj["upper"][once].tobytes()
    assert ar["lower"][once].tobytes() == aj["lower"][once].tobytes() and ar["spread"][once].tobytes() == aj["spread"][once].tobytes()
    assert not ar["rot_spread"][once].any() and ar["rot_spread"][ar["covered"] == 2].min() > 0.0 and sr["degenerate_bones"] == 0
    assert np.isnan(ar["pred"][ar["covered"] == 0]).all() and np.isnan(ar["rot"][ar["covered"] == 0]).all()


def test_the_other_spaces_keep_their_bits_and_allocate_nothing(world):
    s0, a0 = world.run("mean", None)
    s1, a1 = world.run("mean", "joints")
    assert set(a1) - set(a0) == {"fallback"} and set(s1) - set(s0) == {"bone_dev_cm", "single_bone_dev_cm", "degenerate_bones", "blend_space"}
    for k, v in a0.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == a1[k].tobytes() and v.dtype == a1[k].dtype, k
        elif isinstance(v, torch.Tensor):
            assert torch.equal(v, a1[k]), k
    sb, ab = world.run("mean", "bones")
    sb2, ab2 = world.run("mean", "bones", tag=1)
    for k, v in ab.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == ab2[k].tobytes(), k
    for k, v in sb.items():
        assert (v.tobytes() == sb2[k].tobytes()) if isinstance(v, np.ndarray) else v == sb2[k], k
    new = {"rot", "rot_spread", "bone_vectors", "win_q_up", "win_q_lo", "win_R"}
    for a in (a0, a1, ab):
        assert not (new & set(a)), "rotations are kept under \"rot\" only"
    for s in (s0, s1, sb):
        assert "rot_spread_deg" not in s
    sr, ar = world.run("mean", "rot")
    assert new <= set(ar) and set(sr) - set(sb) == {"rot_spread_deg"}
    # the window rows and the single-window figures do not depend on the blend space
    assert torch.equal(ar["win_up"], a0["win_up"]) and torch.equal(ar["win_lo"], a0["win_lo"])
    for k in ("single_all_cm", "single_upper_cm", "single_lower_cm", "single_rot_deg"):
        assert sr[k] == s0[k], k


@pytest.mark.parametrize("blend", ["mean", "triangle"])
def test_summary_figures(world, blend):
    s, a = world.run(blend, "rot")
    cov = a["covered"] > 0
    (_, _, _, rspr64, _), _, _ = _restated(world, a)
    want_deg = float(np.degrees(rspr64[cov]).mean())
    d = np.concatenate([bref.bone_length_dev(a["upper"][cov].reshape(-1, 45), bref.UPPER_WALK, world.L),
                        bref.bone_length_dev(a["lower"][cov].reshape(-1, 24), bref.LOWER_WALK, world.L[14:])], axis=1)
    want_dev = float(d.mean()) * 100
    allj = np.linalg.norm(a["pred"][cov].astype(np.float64) - a["target"][cov], axis=2).mean() * 100
    _, upper, lower, _ = ref.errors_cm(a["upper"][cov], a["lower"][cov], a["target"][cov])
    spread = float(a["spread"][cov].astype(np.float64).mean()) * 100
    print("rot %s: rot_spread %.6f / %.6f deg  bone_dev %.6f / %.6f  all %.6f / %.6f  upper %.6f / %.6f  lower %.6f / %.6f  spread %.6f / %.6f cm"
          % (blend, s["rot_spread_deg"], want_deg, s["bone_dev_cm"], want_dev, s["all_cm"], allj, s["upper_cm"], upper, s["lower_cm"], lower,
             s["spread_cm"], spread))
    # (every frame's float is within 2^-23 |ref| + 1e-7 rad of the restatement, 5.7e-6 degrees; the column sum adds one float rounding)
    assert abs(s["rot_spread_deg"] - want_deg) <= 2.0 ** -22 * want_deg + 1e-5
    assert abs(s["bone_dev_cm"] - want_dev) <= 1e-3 and s["bone_dev_cm"] <= 2e-4
    assert abs(s["all_cm"] - allj) <= 1e-3 and abs(s["upper_cm"] - upper) <= 1e-3 and abs(s["lower_cm"] - lower) <= 1e-3
    assert abs(s["spread_cm"] - spread) <= 1e-3


def test_rot_with_smooth_is_refused(world):
    from mmego_amd import dense
    with pytest.raises(ValueError, match="would not be filtered"):
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, blend_space="rot", smooth=(3, 2, "gauss"))


def _run(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_command_line_writes_rotations_that_reproduce_pred(world):
    """`main.py --infer --dense --stride 3 --blend_space rot --save_pred ...` in a fresh child process: the new line, the new arrays, and
    from the file ALONE -- pred's roots, rot, bone_vectors -- numpy forward kinematics gives pred again."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    path = str(world.tmp / "pred_rot.npz")
    out = _run(["--infer", "--dense", "--stride", "3", "--gt_head_pose", "--data_root", world.data, "--device", "cuda:0", "--seed", "3",
                "--batch_size", "4", "--load_Upper_path", str(world.tmp / "upper.pth"), "--load_Lower_path", str(world.tmp / "lower.pth"),
                "--blend_space", "rot", "--save_pred", path], env)
    assert out.count(LINE) == 1 and "(degenerate bones 0)" in out
    assert out.index("Bone Length Deviation(cm):") < out.index(LINE) < out.index("Dense windows:")
    z = np.load(path)
    today = {"pred", "covered", "spread", "recording", "frame_in_recording", "target", "stride", "blend", "frame_no"}
    assert set(z.files) == today | {"blend_space", "degenerate_bones", "rot", "rot_spread", "bone_vectors"}
    assert str(z["blend_space"]) == "rot" and int(z["degenerate_bones"]) == 0 and int(z["stride"]) == 3
    assert z["pred"].shape == (F, 21, 3) and z["rot"].shape == (F, 20, 4) and z["rot_spread"].shape == (F,) and z["bone_vectors"].shape == (20, 3)
    assert z["rot"].dtype == np.float32 and z["bone_vectors"].dtype == np.float32
    cov = z["covered"] > 0
    assert cov.sum() == F - 7 and np.isnan(z["rot"][~cov]).all() and np.isnan(z["pred"][~cov]).all()
    assert not np.isnan(z["rot"][cov]).any() and not np.isnan(z["rot_spread"]).any()
    s, a = world.run("mean", "rot")
    assert a["pred"].tobytes() == z["pred"].tobytes() and a["rot"].tobytes() == z["rot"].tobytes()
    assert np.array_equal(z["bone_vectors"], world.body)
    assert float(out.split(LINE)[1].split()[0]) == s["rot_spread_deg"]
    # forward kinematics from the file alone, in the 21-joint numbering.  The upper tree hangs from the head (20); the legs hang from
    # the hips as the LOWER net placed them, which is what pred holds at joints 12 and 16 -- so the two upper hip bones (0 -> 12,
    # 0 -> 16) are checked against the upper tree's own walk, not against pred's hips.
    pred, rot, body = z["pred"][cov].astype(np.float64), z["rot"][cov].astype(np.float64), z["bone_vectors"].astype(np.float64)
    pos = np.full_like(pred, np.nan)
    pos[:, 20], pos[:, 12], pos[:, 16] = pred[:, 20], pred[:, 12], pred[:, 16]
    worst = 0.0
    for i in range(len(pred)):
        for b, (p, c) in enumerate(BONES_ALL):
            x = pos[i, p] + rref.matrix(rot[i, b]) @ body[b]
            if c in (12, 16) and b < 14:
                continue                                   # (the upper net's hips: overwritten by the lower net's in pred)
            pos[i, c] = x
    worst = np.abs(pos - pred).max()
    print("FK of the saved rotations over the saved rest bones against the saved pred: worst %.3e m over %d frames" % (worst, len(pred)))
    assert not np.isnan(pos).any() and worst <= 2e-5
