"""GPU: `--metrics full` on the command line, on the tiny synthetic Sample_data tree of tests/test_cli_gpu.py (same .mat keys and layout):
--infer prints the reference's five lines unchanged and first, then the new figures; stage-2 training prints one more line per epoch
and writes the same log files."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.io as scio

from conftest import ROOT

pytestmark = pytest.mark.gpu

REFERENCE_LINES = ("Average Joint Localization Error(cm):", "Average UpperBody Joint Localization Error(cm):",
                   "Average LowerBody Joint Localization Error(cm):", "Average Joint Rotation Error", "Per Joint Localization Error(cm):")
NUMBER = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"


def _make_dataset(root, rng):
    for a in (1, 2):
        for s in (1, 2, 3):
            d = os.path.join(root, "%02d" % a, "s%d" % s)
            os.makedirs(d)
            skel = rng.normal(0, 0.4, (32, 3)) + np.array([0.8, 0.0, 0.2])
            for f in range(23):
                n = int(rng.integers(20, 150))
                pc = np.concatenate([rng.normal([0.8, 0.0, 0.2], 0.4, (n, 3)), rng.uniform(10, 46, (n, 1)), rng.normal(0, 0.4, (n, 1))], 1)
                q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
                imu = np.concatenate([np.tile(q.reshape(1, 9), (20, 1)), rng.normal(size=(20, 6))], 1)
                scio.savemat(os.path.join(d, "frame_%d.mat" % f), {
                    "pc_xyziv_ti2": pc.astype(np.float32), "pc_xyz_key_2": skel + rng.normal(0, 0.01, (32, 3)),
                    "imu_save_l": imu, "R_btc": q, "orientation_imu_img": np.eye(3), "t_R0R": rng.normal(size=(1, 3)),
                    "abcd_ground_2": np.array([[0.0, 0.0, -1.0, 1.0]]), "foot_contact": np.array([[1, 0]])})


def _run(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def _reference_block(out):
    """The reference's five --infer lines as printed: from the first of them to the end of the per-joint array."""
    start = out.index(REFERENCE_LINES[0])
    end = out.index("]", out.index(REFERENCE_LINES[4])) + 1
    block = out[start:end]
    assert all(line in block for line in REFERENCE_LINES)
    return block, out[end:]


def test_infer_prints_the_reference_lines_unchanged_then_the_new_figures(tmp_path):
    import torch
    from mmego_amd import nets
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(0))
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(tmp_path / "train_out"))
    torch.manual_seed(0)
    torch.save(nets.UpperNet().state_dict(), tmp_path / "upper.pth")
    torch.save(nets.LowerNet(64).state_dict(), tmp_path / "lower.pth")
    # (--seed: the loader pads and subsamples the point clouds with numpy's global generator -- two runs see the same data)
    infer = ["--infer", "--gt_head_pose", "--data_root", data, "--device", "cuda:0", "--seed", "3", "--load_Upper_path", str(tmp_path / "upper.pth"),
             "--load_Lower_path", str(tmp_path / "lower.pth")]
    plain, rest_plain = _reference_block(_run(infer, env))
    full, rest = _reference_block(_run(infer + ["--metrics", "full"], env))
    assert plain == full
    assert "Joint Error(cm)" not in rest_plain and "PCK@" not in rest_plain
    values = {}
    for name in ("Root-relative Joint Error(cm)", "Rigid-aligned Joint Error(cm)", "Procrustes-aligned (PA-MPJPE) Joint Error(cm)"):
        m = re.search(re.escape(name) + r": (%s) \(upper (%s), lower (%s)\)" % (NUMBER, NUMBER, NUMBER), rest)
        assert m, (name, rest)
        values[name] = [float(v) for v in m.groups()]
    for name in ("Alignment Rotation(°)", "Alignment Shift(cm)", "Procrustes Scale", "PCK@5cm", "PCK@10cm", "PCK@15cm",
                 "Acceleration Error(cm/frame^2)"):
        m = re.search(r"^" + re.escape(name) + r": (%s)$" % NUMBER, rest, flags=re.M)
        assert m, (name, rest)
        values[name] = [float(m.group(1))]
    for name in ("Per Joint Root-relative Error(cm)", "Per Joint Procrustes-aligned Error(cm)"):
        m = re.search(re.escape(name) + r": \[([^\]]*)\]", rest)
        assert m, (name, rest)
        values[name] = [float(v) for v in m.group(1).split()]
        assert len(values[name]) == 21
    assert all(np.isfinite(v) for vs in values.values() for v in vs)
    assert 0.0 <= values["PCK@5cm"][0] <= values["PCK@10cm"][0] <= values["PCK@15cm"][0] <= 1.0
    assert 0.0 <= values["Alignment Rotation(°)"][0] <= 180.0 and values["Per Joint Root-relative Error(cm)"][0] == 0.0      # (the root itself)


def test_stage_two_training_prints_one_more_line_and_keeps_its_log_files(tmp_path):
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(0))
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    train = ["--train", "--network", "Upper_Net", "--gt_head_pose", "--data_root", data, "--epochs", "1", "--batch_size", "4",
             "--device", "cuda:0", "--seed", "3"]
    plain = _run(train + ["--log_dir", "9201"], env)
    full = _run(train + ["--log_dir", "9202", "--metrics", "full"], env)
    assert "Aligned metrics:" not in plain
    lines = [l for l in full.splitlines() if l.startswith("Aligned metrics:")]
    assert len(lines) == 1 and "PA-MPJPE" in lines[0] and "PCK @5cm" in lines[0] and "nan" not in lines[0].lower()
    assert full.index("Eval_loss:") < full.index("Aligned metrics:")                     # after the existing lines of the epoch
    for name in ("log-eval.txt", "log-loss.txt"):
        a, b = (open(os.path.join(out_dir, "report", idx, name)).read() for idx in ("9201", "9202"))
        assert len(a.splitlines()) == len(b.splitlines()) and "Aligned" not in b, name
