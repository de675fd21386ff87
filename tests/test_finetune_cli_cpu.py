"""CPU: the command line's handling of --finetune_imu / --imu_lr -- every arrangement the mode does not support is refused with a
message before any work starts -- and the C ABI of the head-pose gradient kernels."""
import os

import pytest

import main as cli
from mmego_amd import hip


def _refused(argv, capsys, monkeypatch, world=None):
    if world is None:
        monkeypatch.delenv("WORLD_SIZE", raising=False)
    else:
        monkeypatch.setenv("WORLD_SIZE", str(world))
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_finetune_imu_argument_handling(capsys, monkeypatch):
    base = ["--train", "--network", "Upper_Net", "--finetune_imu"]
    assert "--gt_head_pose" in _refused(base + ["--gt_head_pose"], capsys, monkeypatch)
    assert "Upper_Net only" in _refused(["--train", "--network", "Lower_Net", "--finetune_imu"], capsys, monkeypatch)
    assert "Upper_Net only" in _refused(["--train", "--network", "IMU_Net", "--finetune_imu"], capsys, monkeypatch)
    assert "Upper_Net only" in _refused(["--infer", "--finetune_imu"], capsys, monkeypatch)
    assert "not data parallel" in _refused(base, capsys, monkeypatch, world=2)
    assert "--resume" in _refused(base + ["--resume", "somewhere/epoch0.pth"], capsys, monkeypatch)
    assert "--finetune_imu" in _refused(["--train", "--network", "Upper_Net", "--imu_lr", "1e-4"], capsys, monkeypatch)


def test_finetune_imu_flags_reach_the_config(monkeypatch):
    from mmego_amd.config import Config
    p = cli.build_parser()
    args = p.parse_args(["--train", "--network", "Upper_Net", "--finetune_imu", "--imu_lr", "2e-5"])
    cli.check_finetune(p, args, 1)
    keep = {k: getattr(Config, k, None) for k in ("finetune_imu", "imu_lr", "resume_path")}
    try:
        cli.apply_overrides(args)
        assert Config.finetune_imu is True and Config.imu_lr == 2e-5
        args = p.parse_args(["--train", "--network", "Upper_Net"])
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        assert Config.finetune_imu is False and Config.imu_lr is None           # (imu_lr None: the trainer falls back to Config.lr)
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


def test_pose_gradient_entry_points_are_declared():
    """The three new entry points are in the header (hip.py binds from it) with the argument lists the nets pass."""
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_transform2h_backward"]] == ["stream", "pts", "ldp", "F", "P", "R", "t", "g", "ldg", "g2", "ldg2",
                                                                    "accumulate", "dR", "dt"]
    assert [n for _, n in protos["mmego_head_fk_backward_pose"]][-3:] == ["joints_h", "dRw", "dtw"]
    assert [n for _, n in protos["mmego_head_fk_backward_pose"]][:-3] == [n for _, n in protos["mmego_head_fk_backward"]]
    assert [n for _, n in protos["mmego_head_fk_loss_pose"]][:-2] == [n for _, n in protos["mmego_head_fk_loss"]]
    src = open(os.path.join(os.path.dirname(hip.HEADER), "..", "mmego_amd", "csrc", "geom.hip")).read()
    for name in ("mmego_transform2h_backward", "mmego_head_fk_backward_pose", "mmego_head_fk_loss_pose"):
        assert 'extern "C" int %s(' % name in src
    assert "atomicAdd" not in src.split("transform2h_bwd_kernel")[1].split("__global__")[0]      # a fixed-order reduction, no atomics
