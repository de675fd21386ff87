"""CPU: --pose_noise_deg / --pose_noise_t -- what the parser refuses, how the values reach Config / ConfigDemo, the key the trainers and
the evaluation passes derive per minibatch, mmego_pose_jitter's declaration, what ops.pose_jitter refuses on the host before any
launch, and the statistics of the numpy restatement of the draws (tests/pose_noise_ref.py) under this key derivation."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import main as cli
import pose_noise_ref as pref

FLAGS = ("--pose_noise_deg", "--pose_noise_t")


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("flag", FLAGS)
def test_parser_refusals(capsys, monkeypatch, flag):
    for argv, said in (([flag, "1"], "goes with --train"),
                       (["--train", "--network", "IMU_Net", flag, "1"], "does not go with --network IMU_Net"),
                       (["--infer", "--network", "IMU_Net", flag, "1"], "does not go with --network IMU_Net"),
                       (["--train", "--network", "Upper_Net", "--finetune_imu", flag, "1"], "cannot be combined with --finetune_imu"),
                       (["--train", "--network", "Lower_Net", "--finetune_all", flag, "1"], "cannot be combined with --finetune_all"),
                       (["--infer", "--vis", flag, "1"], "does not go with --vis")):
        err = _refused(argv, capsys, monkeypatch)
        assert flag in err and said in err, argv


@pytest.mark.parametrize("value", ["0", "-0.5", "nan", "inf", "-inf"])
@pytest.mark.parametrize("flag", FLAGS)
def test_a_sigma_that_is_not_finite_and_positive_is_refused(capsys, monkeypatch, flag, value):
    for argv in (["--train", "--network", "Upper_Net"], ["--train", "--network", "Lower_Net"], ["--infer"], ["--infer", "--dense"]):
        err = _refused(argv + [flag + "=" + value], capsys, monkeypatch)
        assert flag in err and "finite and > 0" in err


def test_flags_reach_the_configs():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("pose_noise_deg", "pose_noise_t", "seed", "window_jitter", "point_keep", "point_noise", "point_noise_v", "finetune_imu",
             "finetune_upper", "finetune_all", "imu_lr", "upper_lr", "imu_dropout", "resume_path", "upper_variant", "clip_grad_norm", "ema_decay",
             "gt_head_pose", "dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "metrics")
    keep = {(c, k): getattr(c, k) for c in (Config, ConfigDemo) for k in names if hasattr(c, k)}
    for c in (Config, ConfigDemo):
        assert c.pose_noise_deg is None and c.pose_noise_t is None                 # (the defaults: the head pose as it comes)
    up, low = ["--train", "--network", "Upper_Net"], ["--train", "--network", "Lower_Net"]
    try:
        for argv, deg, t in ((up + ["--gt_head_pose", "--pose_noise_deg", "2"], 2.0, None),
                             (up + ["--pose_noise_t", "0.02"], None, 0.02),
                             (up + ["--upper_variant", "wlocal", "--pose_noise_deg", "2", "--pose_noise_t", "0.02", "--seed", "1"], 2.0, 0.02),
                             (up + ["--resume", "somewhere.pth", "--pose_noise_deg", "0.5"], 0.5, None),
                             (up + ["--window_jitter", "--point_keep", "0.8", "--point_noise", "0.02", "--pose_noise_deg", "1"], 1.0, None),
                             (up + ["--ema_decay", "0.99", "--clip_grad_norm", "1", "--pose_noise_t", "0.05"], None, 0.05),
                             (low + ["--finetune_upper", "--pose_noise_deg", "1", "--pose_noise_t", "0.01"], 1.0, 0.01),
                             (["--infer", "--pose_noise_deg", "5", "--seed", "3"], 5.0, None),
                             (["--infer", "--dense", "--save_pred", "x.npz", "--pose_noise_t", "0.05"], None, 0.05),
                             (low, None, None), (["--infer"], None, None)):
            args = p.parse_args(argv)
            cli.check_finetune(p, args, 1)
            if "--finetune_upper" not in argv:
                cli.check_finetune(p, args, 4)                                     # (data parallel: accepted as well; --finetune_upper is not)
            cli.apply_overrides(args)
            for c in (Config, ConfigDemo):
                assert c.pose_noise_deg == deg and c.pose_noise_t == t, argv
            if "--seed" in argv and "--infer" in argv:
                assert ConfigDemo.seed == 3
    finally:
        for (c, k), v in keep.items():
            setattr(c, k, v)


def test_the_key_is_a_pure_function_of_its_words():
    from mmego_amd import processors
    from mmego_amd.data import _mix64
    key = processors.pose_noise_key
    base = key(1, 2, 3, 0)
    assert base == key(1, 2, 3, 0) == _mix64(1, 2, 3, 0, 0x504F5345) & (2 ** 63 - 1)
    others = [key(2, 2, 3, 0), key(1, 3, 3, 0), key(1, 2, 4, 0), key(1, 2, 3, 1), key(1, 2, 3)]
    assert len({base, *others}) == 6
    assert all(0 <= k < 2 ** 63 for k in [base] + others)
    assert key(1, 0, 3) == _mix64(1, 0, 3, 0x504F5345) & (2 ** 63 - 1)            # the evaluation passes' key: no rank

    class Cfg:
        pose_noise_deg, pose_noise_t, seed = None, None, 7
    assert processors.pose_noise_of(Cfg) is None
    Cfg.pose_noise_t = 0.02
    assert processors.pose_noise_of(Cfg) == (0.0, 0.02, 7)
    Cfg.pose_noise_deg, Cfg.seed = 2, None                                         # (a missing --seed: 0, as --point_noise treats it)
    assert processors.pose_noise_of(Cfg) == (2.0, 0.02, 0)
    assert processors.pose_noise_line((2.0, 0.02, 0)) == "Head Pose Noise: rotation 2.0 deg per axis, translation 0.02 m, seed 0"


def test_pose_jitter_is_declared_as_ops_calls_it():
    from mmego_amd import dense, hip, ops, processors, train_step
    proto = hip.parse_header()["mmego_pose_jitter"]
    assert [n for _, n in proto] == ["stream", "R", "t", "n", "sigma_deg", "sigma_t", "seed_word", "ids", "R_out", "t_out"]
    assert [c for c, _ in proto] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert list(inspect.signature(ops.pose_jitter).parameters) == ["R", "t", "sigma_deg", "sigma_t", "word", "R_out", "t_out", "ids"]
    assert inspect.signature(ops.pose_jitter).parameters["ids"].default is None
    step = inspect.signature(train_step.StageStep.__init__).parameters
    assert step["pose_noise_deg"].default is None and step["pose_noise_t"].default is None
    for fn in (processors._epoch_eval, processors.evaluate_full, dense.dense_infer):
        assert inspect.signature(fn).parameters["pose_noise"].default is None


def test_ops_pose_jitter_refuses_on_the_host():
    """Everything here is refused before the library is touched: CPU tensors stand in for the device's."""
    from mmego_amd import ops
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    R, t, word = f(2, 4, 3, 3), f(2, 4, 3), torch.zeros(1, dtype=torch.int64)
    ok = dict(R=R, t=t, R_out=f(2, 4, 3, 3), t_out=f(2, 4, 3))
    for name, bad in (("R", f(2, 4, 3, 3).double()), ("R", f(2, 4, 9)), ("R", f(3, 3)), ("R", f(2, 4, 3, 6)[..., ::2]), ("t", f(2, 4, 4)),
                      ("t", f(2, 4, 3).half()), ("t", f(2, 4, 6)[..., ::2]), ("R_out", f(2, 4, 3, 3).int()), ("R_out", f(2, 4, 4, 3)),
                      ("t_out", f(3,)), ("t_out", f(2, 3, 4).transpose(1, 2))):
        args = dict(ok, **{name: bad})
        with pytest.raises(ValueError, match="pose_jitter: %s is a contiguous fp32 tensor" % name):
            ops.pose_jitter(args["R"], args["t"], 1.0, 0.02, word, args["R_out"], args["t_out"])
    for name, bad in (("t", f(2, 5, 3)), ("R_out", f(2, 5, 3, 3)), ("t_out", f(1, 4, 3)), ("R", f(0, 3, 3))):
        args = dict(ok, **{name: bad})
        with pytest.raises(ValueError, match="one and the same number of poses"):
            ops.pose_jitter(args["R"], args["t"], 1.0, 0.02, word, args["R_out"], args["t_out"])
    for bad in (word, word.int(), 5, None, torch.zeros(0, dtype=torch.int64)):   # (a host word included: the kernel reads it on the device)
        with pytest.raises(TypeError, match="int64 device seed word"):
            ops.pose_jitter(R, t, 1.0, 0.02, bad, ok["R_out"], ok["t_out"])


@pytest.mark.parametrize("word", [0, 1, 12345678901234567, 2 ** 63 - 1])
def test_statistics_of_the_restated_draws(word):
    """What tests/test_pose_noise_gpu.py asks of the kernel's recovered draws, asked of the restatement's z at the same n."""
    n = 65536
    z = pref.draws(word, np.arange(n)).astype(np.float64)
    N = 3 * n
    assert np.abs(z).max() <= 3.4642
    for half in (z[:, :3], z[:, 3:]):
        assert abs(half.mean()) <= 5 / np.sqrt(N) and abs(half.var() - 1.0) <= 5 * np.sqrt(1.7 / N)
    assert np.abs(np.corrcoef(z.T) - np.eye(6)).max() < 4 / np.sqrt(n)
    # and the recipe on top of them: a rotation, by no more than 6 sigma_deg; a shift by no more than 3.47 sigma_t
    E = pref.rotations(2.0, z[:4096].astype(np.float32))
    assert np.abs(E @ E.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    assert np.degrees(np.linalg.norm(pref.rotation_vectors(E), axis=1)).max() <= 6 * 2.0
    R, t = np.tile(np.eye(3, dtype=np.float32), (8, 1, 1)), np.zeros((8, 3), np.float32)
    Rn, tn = pref.pose_jitter(R, t, 0.0, 0.05, word)
    assert np.array_equal(Rn, R) and np.abs(tn).max() <= 3.47 * 0.05 and np.abs(tn).min() > 0
    again = pref.pose_jitter(R, t, 0.0, 0.05, word, ids=np.arange(8) + 2 ** 32)
    assert np.array_equal(tn, again[1])                                            # (the draw number is the id's low 32 bits)
