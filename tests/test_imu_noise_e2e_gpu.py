"""GPU: --imu_noise_* / --imu_bias_* end to end on the synthetic Sample_data tree of tests/test_dense_bones_gpu.py (recordings of 23, 20,
7 and 41 frames, frame_no = 20: three training windows and one test window; nets from torch.manual_seed, the IMU_Net among them): the
command line's stage-1 training run against its own --resume, dense inference against itself at two minibatch sizes, the evaluator's
output file, and plain --infer.  The command line runs in this process (main.main(argv)); the configuration classes are put back."""
import glob
import os

import numpy as np
import pytest
import torch

import main as cli
from test_dense_bones_gpu import F, T, _make_dataset

pytestmark = pytest.mark.gpu

SIGMAS = (1.0, 0.05, 0.01, 2.0, 0.2, 0.02)
NOISE = (SIGMAS, 1)
NAMES = ("imu_noise_rot_deg", "imu_noise_acc", "imu_noise_gyro", "imu_bias_rot_deg", "imu_bias_acc", "imu_bias_gyro")
FLAGS = [v for n, s in zip(NAMES, SIGMAS) for v in ("--" + n, repr(s))]
LINE = ("IMU Noise: white rotation 1.0 deg per axis, accelerometer 0.05, gyroscope 0.01; bias rotation 2.0 deg per axis, accelerometer 0.2, "
        "gyroscope 0.02; seed 1")
TODAY = {"pred", "covered", "spread", "recording", "frame_in_recording", "target", "stride", "blend", "frame_no"}


class _World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    assert torch.cuda.is_available()
    from mmego_amd import nets
    w = _World()
    w.tmp = tmp_path_factory.mktemp("imu_noise")
    w.data = str(w.tmp / "Sample_data")
    _make_dataset(w.data, np.random.default_rng(0))
    torch.manual_seed(0)
    w.up, w.lo = nets.UpperNet().to("cuda:0").eval(), nets.LowerNet(64).to("cuda:0").eval()
    w.imu = nets.IMUNet(15, 9, 512, 2, True, 0.1).to("cuda:0").eval()
    torch.save(w.up.state_dict(), w.tmp / "upper.pth")
    torch.save(w.lo.state_dict(), w.tmp / "lower.pth")
    torch.save(w.imu.state_dict(), w.tmp / "imu.pth")
    w.where = ["--data_root", w.data, "--device", "cuda:0"]
    w.common = w.where + ["--load_IMU_path", str(w.tmp / "imu.pth"), "--load_Upper_path", str(w.tmp / "upper.pth"),
                          "--load_Lower_path", str(w.tmp / "lower.pth")]
    return w


@pytest.fixture()
def configs(monkeypatch):
    """main.apply_overrides writes class attributes: both classes are put back as they were."""
    from mmego_amd.config import Config, ConfigDemo
    keep = [(c, dict(vars(c))) for c in (Config, ConfigDemo)]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for c in (Config, ConfigDemo):
        c.gt_head_pose = False        # (apply_overrides only ever sets it: a command line run earlier in the process may have left it on)
    yield
    for c, was in keep:
        for k in [k for k in vars(c) if k not in was]:
            delattr(c, k)
        for k, v in was.items():
            if not k.startswith("__") and vars(c).get(k, None) is not v:
                setattr(c, k, v)


def _train(world, monkeypatch, out, argv):
    """`main.py --train --network IMU_Net ...` with its directories under ``out`` -> the checkpoints it left, by file name."""
    from mmego_amd import processors
    monkeypatch.setattr(processors, "_TRAIN_DIR", str(world.tmp / out))
    cli.main(["--train", "--network", "IMU_Net", "--batch_size", "2", "--seed", "1", "--log_dir", "7"] + world.where + argv)
    torch.cuda.synchronize()
    return {os.path.basename(p): p for p in glob.glob(str(world.tmp / out / "model" / "7" / "*.pth")) if not p.endswith(".train_state.pth")}


def _same_weights(a, b):
    a, b = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    assert a.keys() == b.keys()
    return all(torch.equal(a[k], b[k]) for k in a)


def test_training_resumes_the_same_sequence(world, configs, monkeypatch, capsys):
    two = _train(world, monkeypatch, "two", FLAGS + ["--epochs", "2"])
    said = capsys.readouterr().out
    assert said.count("[mmego_amd] IMU noise: white rotation 1 deg per axis, accelerometer 0.05, gyroscope 0.01; bias per window rotation 2 deg "
                      "per axis, accelerometer 0.2, gyroscope 0.02") == 1
    one = _train(world, monkeypatch, "one", FLAGS + ["--epochs", "1"])
    (first,) = [n for n in one if n.startswith("epoch0_")]
    again = _train(world, monkeypatch, "one", FLAGS + ["--epochs", "2", "--resume", one[first]])
    assert "resumed from" in capsys.readouterr().out
    (last,) = [n for n in two if n.startswith("epoch1_")]
    assert _same_weights(two[last], again[last]), "one epoch and --resume: the second epoch's draws continue the sequence"
    plain = _train(world, monkeypatch, "plain", ["--epochs", "1"])
    assert "IMU noise" not in capsys.readouterr().out
    assert not _same_weights(one[first], plain[first]), "without the flags: other weights"
    sd = torch.load(one[first], map_location="cpu")
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    # the train state beside the checkpoint keeps exactly today's keys: no new saved state
    ts = torch.load(one[first][:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    assert set(ts) == {"epoch", "model", "optimizer", "rng", "dropout_counter", "early"}
    tp = torch.load(plain[first][:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    assert set(ts["optimizer"]) == set(tp["optimizer"])


@pytest.fixture(scope="module")
def dense(world):
    """The dense passes the tests share: ``run(batch_size, imu_noise)`` -> (summary, arrays), computed once; ``fresh`` computes again."""
    from mmego_amd import processors
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import PosePC
    from mmego_amd.dense import dense_infer
    np.random.seed(3)
    ds = PosePC(train=False, vis=True, keep_frames=True, batch_length=T, root=world.data)
    keep = ConfigDemo.gt_head_pose
    ConfigDemo.gt_head_pose = True                          # (_Base only: the passes below are handed the IMU_Net)
    try:
        base = processors._Base(ConfigDemo, make_dirs=False)
    finally:
        ConfigDemo.gt_head_pose = keep
    d = _World()
    d.runs = {}

    def fresh(batch_size, noise):
        more = {} if noise is None else dict(imu_noise=noise)
        return dense_infer(base, world.imu, world.up, world.lo, ds, 3, batch_size=batch_size, **more)

    def run(batch_size, noise):
        if (batch_size, noise) not in d.runs:
            d.runs[(batch_size, noise)] = fresh(batch_size, noise)
        return d.runs[(batch_size, noise)]
    d.fresh, d.run, d.base, d.ds = fresh, run, base, ds
    return d


def test_dense_inference_does_not_depend_on_the_minibatch(world, dense):
    """Twice the same arrays; the same skeletons at two minibatch sizes (the draw numbers are the row's global frame and the plan's window,
    not their places in the minibatch), within the project's 2e-5 m for two minibatch sizes; and other skeletons than the noise-free
    pass's."""
    from mmego_amd.dense import dense_infer
    s4, a4 = dense.run(4, NOISE)
    s4b, a4b = dense.fresh(4, NOISE)
    for k in ("pred", "upper", "lower", "spread"):
        assert a4[k].tobytes() == a4b[k].tobytes(), k
    assert torch.equal(a4["win_up"], a4b["win_up"]) and torch.equal(a4["win_lo"], a4b["win_lo"]) and s4["all_cm"] == s4b["all_cm"]
    s3, a3 = dense.run(3, NOISE)
    cov = a4["covered"] > 0
    assert cov.sum() == F - 7 and np.array_equal(np.isnan(a3["pred"]), np.isnan(a4["pred"]))
    worst = np.abs(a4["pred"][cov].astype(np.float64) - a3["pred"][cov]).max()
    print("batch_size 4 against 3 under IMU noise: largest difference %.3g m (bound 2e-5)" % worst)
    assert worst <= 2e-5
    s0, a0 = dense.run(4, None)
    moved = np.abs(a4["pred"][cov].astype(np.float64) - a0["pred"][cov]).max()
    print("IMU noise moved a joint by up to %.3g m" % moved)
    assert moved > 1e-4 and set(s0) == set(s4) and set(a0) == set(a4)
    with pytest.raises(ValueError, match="imu_noise"):
        dense_infer(dense.base, None, world.up, world.lo, dense.ds, 3, batch_size=4, imu_noise=NOISE)


def _infer(world, argv):
    cli.main(["--infer", "--seed", "1"] + world.common + argv)
    torch.cuda.synchronize()


def test_evaluator_writes_the_extra_keys(world, configs, capsys):
    path, plain = str(world.tmp / "noisy.npz"), str(world.tmp / "plain.npz")
    dense_args = ["--dense", "--stride", "3", "--batch_size", "4"]
    _infer(world, dense_args + ["--save_pred", path] + FLAGS)
    said = capsys.readouterr().out
    assert said.count(LINE) == 1 and said.rstrip().splitlines()[-1] == LINE
    _infer(world, dense_args + ["--save_pred", plain])
    assert "IMU Noise" not in capsys.readouterr().out
    z, p = np.load(path), np.load(plain)
    assert set(p.files) == TODAY and set(z.files) == TODAY | set(NAMES) | {"imu_noise_seed"}
    assert tuple(float(z[n]) for n in NAMES) == SIGMAS and int(z["imu_noise_seed"]) == 1
    assert z["pred"].shape == p["pred"].shape == (F, 21, 3) and z["pred"].tobytes() != p["pred"].tobytes()
    # a subset of the flags: the others are written as 0
    _infer(world, dense_args + ["--save_pred", path, "--imu_bias_acc", "0.2"])
    assert capsys.readouterr().out.rstrip().splitlines()[-1] == (
        "IMU Noise: white rotation 0.0 deg per axis, accelerometer 0.0, gyroscope 0.0; bias rotation 0.0 deg per axis, accelerometer 0.2, "
        "gyroscope 0.0; seed 1")
    z = np.load(path)
    assert tuple(float(z[n]) for n in NAMES) == (0.0, 0.0, 0.0, 0.0, 0.2, 0.0)


def test_plain_infer_prints_the_line_last(world, configs, capsys):
    shown = ("Average", "Per Joint", "IMU Noise", " ", "[")
    outs = []
    for _ in range(2):
        _infer(world, FLAGS)
        outs.append([l for l in capsys.readouterr().out.splitlines() if l.startswith(shown)])
    assert outs[0] == outs[1] and outs[0][-1] == LINE
    assert sum(l.startswith("Average Joint Localization Error(cm)") for l in outs[0]) == 1
    _infer(world, [])
    plain = [l for l in capsys.readouterr().out.splitlines() if l.startswith(shown)]
    assert not any("IMU Noise" in l for l in plain)
    # the reference's lines print as always: the same lines in the same order, then the one line more
    head = lambda lines: [l.split(":")[0] for l in lines if l.startswith(("Average", "Per Joint"))]
    assert head(plain) == head(outs[0]) and len(head(plain)) >= 4
    first = lambda lines: [l for l in lines if l.startswith("Average Joint Localization Error(cm)")]
    assert len(first(plain)) == 1 and first(plain) != first(outs[0]), "the noise changes the reported error"
