"""CPU: --imu_noise_* / --imu_bias_* -- what the parser refuses, how the values reach Config / ConfigDemo, the key the trainers and the
evaluation passes derive per minibatch, mmego_imu_jitter's declaration, what ops.imu_jitter and the steps refuse on the host before any
launch, and the statistics of the numpy restatement of the draws (tests/imu_noise_ref.py)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import main as cli
import imu_noise_ref as iref

FLAGS = ("--imu_noise_rot_deg", "--imu_noise_acc", "--imu_noise_gyro", "--imu_bias_rot_deg", "--imu_bias_acc", "--imu_bias_gyro")
NAMES = tuple(f[2:] for f in FLAGS)


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("flag", FLAGS)
def test_parser_refusals(capsys, monkeypatch, flag):
    for argv, said in (([flag, "1"], "goes with --train or --infer"),
                       (["--infer", "--vis", flag, "1"], "does not go with --vis"),
                       (["--infer", "--gt_head_pose", flag, "1"], "cannot be combined with --gt_head_pose"),
                       (["--infer", "--dense", "--gt_head_pose", flag, "1"], "cannot be combined with --gt_head_pose"),
                       (["--train", "--network", "Upper_Net", "--gt_head_pose", flag, "1"], "cannot be combined with --gt_head_pose"),
                       (["--train", "--network", "Lower_Net", "--gt_head_pose", flag, "1"], "cannot be combined with --gt_head_pose")):
        err = _refused(argv, capsys, monkeypatch)
        assert flag in err and said in err, argv


@pytest.mark.parametrize("value", ["0", "-0.5", "nan", "inf", "-inf"])
@pytest.mark.parametrize("flag", FLAGS)
def test_a_sigma_that_is_not_finite_and_positive_is_refused(capsys, monkeypatch, flag, value):
    for argv in (["--train", "--network", "IMU_Net"], ["--train", "--network", "Upper_Net"], ["--infer"], ["--infer", "--dense"]):
        err = _refused(argv + [flag + "=" + value], capsys, monkeypatch)
        assert flag in err and "finite and > 0" in err


def test_flags_reach_the_configs():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    keep = [(c, dict(vars(c))) for c in (Config, ConfigDemo)]
    for c in (Config, ConfigDemo):
        assert all(getattr(c, n) is None for n in NAMES)                           # (the defaults: the samples as they come)
    imu, up, low = (["--train", "--network", n] for n in ("IMU_Net", "Upper_Net", "Lower_Net"))
    all_six = [v for f, s in zip(FLAGS, ("1", "0.1", "0.01", "2", "0.2", "0.02")) for v in (f, s)]
    try:
        for argv, want in ((imu + ["--imu_noise_acc", "0.1"], (None, 0.1, None, None, None, None)),
                           (imu + ["--gt_head_pose", "--imu_bias_gyro", "0.02"], (None, None, None, None, None, 0.02)),   # (stage 1 reads no pose)
                           (imu + all_six + ["--seed", "1", "--imu_dropout", "0.1", "--clip_grad_norm", "1", "--ema_decay", "0.99",
                                             "--window_jitter", "--lr_schedule", "cosine"], (1.0, 0.1, 0.01, 2.0, 0.2, 0.02)),
                           (imu + ["--resume", "somewhere.pth", "--imu_bias_rot_deg", "2"], (None, None, None, 2.0, None, None)),
                           (up + ["--finetune_imu", "--imu_noise_rot_deg", "1", "--imu_bias_acc", "0.2"], (1.0, None, None, None, 0.2, None)),
                           (up + ["--pose_noise_deg", "1", "--point_keep", "0.8", "--point_noise", "0.02", "--imu_noise_gyro", "0.01"],
                            (None, None, 0.01, None, None, None)),
                           (low + ["--finetune_all"] + all_six, (1.0, 0.1, 0.01, 2.0, 0.2, 0.02)),
                           (low + ["--imu_bias_rot_deg", "0.5"], (None, None, None, 0.5, None, None)),
                           (["--infer", "--seed", "3"] + all_six, (1.0, 0.1, 0.01, 2.0, 0.2, 0.02)),
                           (["--infer", "--dense", "--save_pred", "x.npz", "--seed", "3", "--imu_noise_acc", "0.05"],
                            (None, 0.05, None, None, None, None)),
                           (imu, (None,) * 6), (["--infer"], (None,) * 6)):
            args = p.parse_args(argv)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            for c in (Config, ConfigDemo):
                assert tuple(getattr(c, n) for n in NAMES) == want, argv
            if "--infer" in argv and "--seed" in argv:
                assert ConfigDemo.seed == 3
    finally:
        for c, was in keep:
            for k in [k for k in vars(c) if k not in was]:
                delattr(c, k)
            for k, v in was.items():
                if not k.startswith("__") and vars(c).get(k, None) is not v:
                    setattr(c, k, v)


def test_the_key_is_a_pure_function_of_its_words():
    from mmego_amd import processors
    from mmego_amd.data import _mix64
    key = processors.imu_noise_key
    base = key(1, 2, 3, 0)
    assert base == key(1, 2, 3, 0) == _mix64(1, 2, 3, 0, 0x494D554E) & (2 ** 63 - 1)
    others = [key(2, 2, 3, 0), key(1, 3, 3, 0), key(1, 2, 4, 0), key(1, 2, 3, 1), key(1, 2, 3)]
    assert len({base, *others}) == 6
    assert all(0 <= k < 2 ** 63 for k in [base] + others)
    assert key(1, 0, 3) == _mix64(1, 0, 3, 0x494D554E) & (2 ** 63 - 1)            # the evaluation passes' key: no rank
    assert key(None, 2, 3, 0) == key(0, 2, 3, 0)                                   # (a missing --seed is 0)
    # a salt of its own: a run under both options draws its head-pose noise and its IMU noise from different keys
    for words in ((1, 2, 3, 0), (0, 0, 0), (7, 1, 5, 3)):
        assert key(*words) != processors.pose_noise_key(*words)

    class Cfg:
        seed = 7
    assert processors.imu_noise_of(Cfg) is None
    Cfg.imu_bias_acc = 0.2
    assert processors.imu_noise_of(Cfg) == ((0.0, 0.0, 0.0, 0.0, 0.2, 0.0), 7)
    Cfg.imu_noise_rot_deg, Cfg.seed = 1, None
    assert processors.imu_noise_of(Cfg) == ((1.0, 0.0, 0.0, 0.0, 0.2, 0.0), 0)
    assert processors.imu_noise_line(((1.0, 0.0, 0.0, 0.0, 0.2, 0.0), 0)) == (
        "IMU Noise: white rotation 1.0 deg per axis, accelerometer 0.0, gyroscope 0.0; bias rotation 0.0 deg per axis, accelerometer 0.2, "
        "gyroscope 0.0; seed 0")


def test_imu_jitter_is_declared_as_ops_calls_it():
    from mmego_amd import dense, hip, ops, processors, train_step
    proto = hip.parse_header()["mmego_imu_jitter"]
    assert [n for _, n in proto] == ["stream", "imu", "n_rows", "T", "S", "noise_rot_deg", "noise_acc", "noise_gyro", "bias_rot_deg",
                                     "bias_acc", "bias_gyro", "seed_word", "row_ids", "win_ids", "out"]
    assert [c for c, _ in proto] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int] + [ctypes.c_double] * 6 + [
        ctypes.c_void_p] * 4
    sig = inspect.signature(ops.imu_jitter).parameters
    assert list(sig) == ["imu", "sigmas", "word", "out", "T", "row_ids", "win_ids"]
    assert all(sig[n].default is None for n in ("T", "row_ids", "win_ids"))
    for step in (train_step.StageStep, train_step.ImuStep):
        assert inspect.signature(step.__init__).parameters["imu_noise"].default is None
    for fn in (processors._epoch_eval, processors.evaluate_full, dense.dense_infer):
        assert inspect.signature(fn).parameters["imu_noise"].default is None


def test_ops_imu_jitter_refuses_on_the_host():
    """Everything here is refused before the library is touched: CPU tensors stand in for the device's."""
    from mmego_amd import ops
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    imu, word, sig = f(2, 3, 20, 15), torch.zeros(1, dtype=torch.int64), (1.0, 0.1, 0.01, 2.0, 0.2, 0.02)
    for name, bad in (("imu", f(2, 3, 20, 15).double()), ("imu", f(2, 3, 20, 16)), ("imu", f(20, 15)), ("imu", f(2, 3, 20, 30)[..., ::2]),
                      ("out", f(2, 3, 20, 15).half()), ("out", f(2, 3, 15, 20).transpose(2, 3)), ("out", None)):
        args = dict(imu=imu, out=f(2, 3, 20, 15))
        args[name] = bad
        with pytest.raises(ValueError, match="imu_jitter: %s is a contiguous fp32 tensor" % name):
            ops.imu_jitter(args["imu"], sig, word, args["out"])
    with pytest.raises(ValueError, match="differ in shape"):
        ops.imu_jitter(imu, sig, word, f(2, 4, 20, 15))
    for T in (4, 0, -1):                                                            # (six frames are no whole windows of four)
        with pytest.raises(ValueError, match="whole windows"):
            ops.imu_jitter(imu, sig, word, f(2, 3, 20, 15), T=T)
    with pytest.raises(ValueError, match="whole windows"):
        ops.imu_jitter(f(0, 3, 20, 15), sig, word, f(0, 3, 20, 15))
    for bad in ((0.0,) * 6, (1.0,) * 5, (1.0,) * 7, (-1.0, 0, 0, 0, 0, 0), (float("nan"), 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, float("inf"))):
        with pytest.raises(ValueError, match="six finite values"):
            ops.imu_jitter(imu, bad, word, f(2, 3, 20, 15))
    for bad in (word, word.int(), 5, None, torch.zeros(0, dtype=torch.int64)):     # (a host word included: the kernel reads it on the device)
        with pytest.raises(TypeError, match="int64 device seed word"):
            ops.imu_jitter(imu, sig, bad, f(2, 3, 20, 15))


def test_the_steps_refuse_bad_sigmas_before_anything_else():
    from mmego_amd.train_step import ImuStep, StageStep
    for bad in ((0.0,) * 6, (1.0,) * 5, (-1.0, 0, 0, 0, 0, 0), (float("nan"),) * 6, (float("inf"), 0, 0, 0, 0, 0), 1.0):
        with pytest.raises(ValueError, match="imu_noise"):
            ImuStep.__new__(ImuStep)._init_imu_noise(bad, "cpu")
    for kw in (dict(imu_net=None), dict(imu_net=object(), pose=(None, None))):      # the recorded pose; somebody else's pose
        with pytest.raises(ValueError, match="imu_noise perturbs what the stage's own IMU_Net reads"):
            StageStep("upper", None, kw.pop("imu_net"), imu_noise=(1.0, 0, 0, 0, 0, 0), **kw)


@pytest.mark.parametrize("word", [0, 12345678901234567, 2 ** 63 - 1])
def test_statistics_of_the_restated_draws(word):
    """What tests/test_imu_noise_gpu.py asks of the kernel's recovered draws, asked of the restatement's z at the same number of samples."""
    rows, S, T = 4096, 20, 4
    zs = iref.sample_draws(word, rows, S).astype(np.float64)
    zw = iref.draws(word, iref.SALT_WINDOW, np.arange(rows * S)).astype(np.float64)
    for z in (zs, zw):
        assert np.abs(z).max() <= 3.4642
        for group in (z[:, :3], z[:, 3:6], z[:, 6:]):
            N = group.size
            assert N >= 2e5 and abs(group.mean()) <= 5 / np.sqrt(N) and abs(group.var() - 1.0) <= 5 * np.sqrt(1.7 / N)
        assert np.abs(np.corrcoef(z.T) - np.eye(9)).max() < 4 / np.sqrt(len(z))
    assert np.abs(np.corrcoef(zs.T, zw.T)[:9, 9:]).max() < 4 / np.sqrt(len(zs))     # the two streams do not follow each other
    # every sample of a window sees one z_w; the draw numbers are the ids' low 32 bits
    w = iref.window_draws(word, 8, T, S)
    assert w.shape == (8 * S, 9) and (w[:T * S] == w[0]).all() and (w[T * S:] == w[T * S]).all() and (w[0] != w[T * S]).any()
    assert np.array_equal(iref.window_draws(word, 8, T, S, win_ids=np.array([5, 2 ** 32 + 5])), np.repeat(w[:1] * 0 + iref.draws(
        word, iref.SALT_WINDOW, [5]), 8 * S, axis=0))
    assert np.array_equal(iref.sample_draws(word, 2, S, row_ids=np.array([3, 3])), np.tile(iref.sample_draws(word, 4, S)[3 * S:], (2, 1)))
