"""CPU: --point_noise / --point_noise_v -- the statistics of the numpy restatement of mmego_pack_frames_noise's draws
(tests/point_noise_ref.py), the entry point's declaration against what ops.pack_frames_noise passes, the command line's handling of the
two flags and FrameStore's refusal of bad values."""
import ctypes
import inspect

import numpy as np
import pytest

import frame_pack_ref as ref
import main as cli
import point_noise_ref as nref

BAR = 0.03                             # on |mean|, |std - 1| and every correlation, at 160 x 150 = 24 000 draws per component (the
                                       # standard error of the mean is 0.0065, of the std 0.004, of a correlation 0.0065)


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 40 + 7])
def test_statistics_of_the_draws(seed):
    z = np.stack([nref.noise_z(150, q, seed) for q in range(160)]).astype(np.float64)          # [160 frames, 150 returns, 4 components]
    flat = z.reshape(-1, 4)
    mean, std, top = flat.mean(axis=0), flat.std(axis=0), np.abs(flat).max()
    corr = np.corrcoef(flat.T)
    cross = np.abs(corr[~np.eye(4, dtype=bool)]).max()
    lag = max(abs(np.corrcoef(z[:, :-1, c].ravel(), z[:, 1:, c].ravel())[0, 1]) for c in range(4))
    print("seed %d: |mean| %.4f  |std - 1| %.4f  max |z| %.4f  cross %.4f  lag-1 %.4f"
          % (seed, np.abs(mean).max(), np.abs(std - 1).max(), top, cross, lag))
    assert (np.abs(mean) <= BAR).all() and (np.abs(std - 1.0) <= BAR).all()
    assert top <= 2.0 * np.sqrt(3.0)
    assert cross <= BAR and lag <= BAR


def test_the_support_is_the_recipes():
    """s_c = 0 and s_c = 4 (2^22 - 1), the ends of the sum, lie within 2 sqrt(3) (1 + 2^-22) of 0 as fp32 values, almost symmetrically."""
    lo, hi = np.float32(0 - 8388606) * nref.SCALE, np.float32(4 * (2 ** 22 - 1) - 8388606) * nref.SCALE
    assert -lo == hi and float(hi) <= 2.0 * np.sqrt(3.0) * (1.0 + 2.0 ** -22)


def test_sigma_zero_copies_and_intensity_is_left_alone():
    raw = np.random.default_rng(0).normal(size=(40, 5)).astype(np.float32)
    raw[3, 0] = raw[5, 4] = -0.0
    same = nref.perturb(raw, 2, 9, 0.0, 0.0)
    assert np.array_equal(same.view(np.uint32), raw.view(np.uint32))
    xyz = nref.perturb(raw, 2, 9, 0.05, 0.0)
    assert np.array_equal(xyz[:, 3:].view(np.uint32), raw[:, 3:].view(np.uint32)) and (xyz[:, :3] != raw[:, :3]).all()
    vel = nref.perturb(raw, 2, 9, 0.0, 0.3)
    assert np.array_equal(vel[:, :4].view(np.uint32), raw[:, :4].view(np.uint32)) and (vel[:, 4] != raw[:, 4]).all()
    # the packing is frame_pack_ref's: the same returns in the same slots
    pts, off = np.concatenate([raw, raw]), np.array([0, 40, 80])
    out, who = nref.pack_frames_noise(pts, off, [1, 0, 1], 16, 40, 0.5, 9, 0.05, 0.3)
    assert np.array_equal(who, ref.pack_frames(pts, off, [1, 0, 1], 16, 40, 0.5, 9)[1])
    assert not np.array_equal(out[0], out[2])                                     # a frame listed twice: two draws


def test_pack_frames_noise_is_declared_as_ops_calls_it():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    plain, noise = protos["mmego_pack_frames"], protos["mmego_pack_frames_noise"]
    assert [n for _, n in noise] == ["stream", "pts", "frame_off", "frame_idx", "nout", "pc_no", "max_n", "keep_p", "seed", "sigma_xyz",
                                     "sigma_v", "out"]
    assert noise[:9] == plain[:9] and noise[11] == plain[9]                         # mmego_pack_frames' parameters, the sigmas before out
    assert noise[8][0] is ctypes.c_ulonglong and noise[9][0] is ctypes.c_float and noise[10][0] is ctypes.c_float
    assert list(inspect.signature(ops.pack_frames_noise).parameters) == ["pts", "frame_off", "frame_idx", "out", "max_n", "keep_p", "seed",
                                                                         "sigma_xyz", "sigma_v"]


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("flag", ["--point_noise", "--point_noise_v"])
def test_flags_are_refused_outside_training(capsys, monkeypatch, flag):
    for argv in (["--infer", flag, "0.02"], [flag, "0.02"], ["--train", "--infer", "--network", "Upper_Net", flag, "0.02"]):
        assert "go with --train only" in _refused(argv, capsys, monkeypatch), argv


@pytest.mark.parametrize("flag", ["--point_noise", "--point_noise_v"])
def test_flags_are_refused_for_stage_1(capsys, monkeypatch, flag):
    err = _refused(["--train", "--network", "IMU_Net", flag, "0.02"], capsys, monkeypatch)
    assert flag + " does not go with --network IMU_Net" in err


@pytest.mark.parametrize("value", ["0", "-0.5", "nan", "inf", "-inf"])
@pytest.mark.parametrize("flag", ["--point_noise", "--point_noise_v"])
def test_a_sigma_that_is_not_finite_and_positive_is_refused(capsys, monkeypatch, flag, value):
    for net in ("Upper_Net", "Lower_Net"):
        assert "finite and > 0" in _refused(["--train", "--network", net, flag + "=" + value], capsys, monkeypatch)


def test_flags_reach_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    names = ("window_jitter", "point_keep", "point_noise", "point_noise_v", "seed", "finetune_imu", "finetune_upper", "finetune_all", "imu_lr",
             "upper_lr", "imu_dropout", "resume_path", "upper_variant", "clip_grad_norm")
    keep = {k: getattr(Config, k, None) for k in names}
    assert Config.point_noise is None and Config.point_noise_v is None             # (the defaults: no noise, DeviceArrays as before)
    up, low = ["--train", "--network", "Upper_Net"], ["--train", "--network", "Lower_Net"]
    try:
        for argv, xyz, vel in ((up + ["--point_noise", "0.02"], 0.02, None),
                               (up + ["--point_noise_v", "0.1"], None, 0.1),
                               (up + ["--point_noise", "0.02", "--point_noise_v", "0.1", "--seed", "1"], 0.02, 0.1),
                               (up + ["--point_keep", "0.8", "--window_jitter", "--point_noise", "0.05"], 0.05, None),
                               (up + ["--upper_variant", "wlocal", "--point_noise", "0.02"], 0.02, None),
                               (up + ["--finetune_imu", "--point_noise_v", "0.3"], None, 0.3),
                               (up + ["--resume", "somewhere.pth", "--point_noise", "0.02"], 0.02, None),
                               (low + ["--finetune_upper", "--point_noise", "0.02"], 0.02, None),
                               (low + ["--finetune_all", "--point_noise", "0.02", "--point_noise_v", "0.2"], 0.02, 0.2),
                               (low, None, None)):
            args = p.parse_args(argv)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.point_noise == xyz and Config.point_noise_v == vel, argv
            assert Config.point_keep == (0.8 if "--point_keep" in argv else None) and Config.window_jitter is ("--window_jitter" in argv)
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


class _NoFrames:
    """What FrameStore looks at before it checks its options."""
    frame_packed_, vis, train = np.zeros((0, 128, 6), np.float32), False, True


@pytest.mark.parametrize("bad", [0, 0.0, -0.05, float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("name", ["point_noise", "point_noise_v"])
def test_frame_store_refuses_a_bad_sigma(name, bad):
    from mmego_amd.data import FrameStore
    with pytest.raises(ValueError, match=name + " is a standard deviation"):
        FrameStore(_NoFrames(), "cpu", **{name: bad})
