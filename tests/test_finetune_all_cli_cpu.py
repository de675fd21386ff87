"""CPU: the command line's handling of --finetune_all (stage 3 training IMU_Net, Upper_Net and Lower_Net together) -- the accepted
form reaches the config, every arrangement the mode does not support is refused with a message before any work starts -- and the C ABI
of the accumulating kinematics backward that the three-net step turns on."""
import os

import pytest

import main as cli
from mmego_amd import hip

BASE = ["--train", "--network", "Lower_Net", "--finetune_all"]
KEYS = ("finetune_all", "finetune_upper", "upper_lr", "finetune_imu", "imu_lr", "imu_dropout", "clip_grad_norm", "resume_path")


def _refused(argv, capsys, monkeypatch, world=None):
    if world is None:
        monkeypatch.delenv("WORLD_SIZE", raising=False)
    else:
        monkeypatch.setenv("WORLD_SIZE", str(world))
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_finetune_all_flags_reach_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    keep = {k: getattr(Config, k, None) for k in KEYS}
    try:
        args = p.parse_args(["--train", "--network", "Lower_Net"])
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        off = {k: getattr(Config, k, None) for k in KEYS}
        assert off == dict(finetune_all=False, finetune_upper=False, upper_lr=None, finetune_imu=False, imu_lr=None, imu_dropout=None,
                           clip_grad_norm=None, resume_path=None)
        args = p.parse_args(BASE + ["--upper_lr", "2e-5", "--imu_lr", "1e-5", "--imu_dropout", "0.25", "--clip_grad_norm", "inf",
                                    "--load_IMU_path", "a.pth", "--load_Upper_path", "b.pth", "--data_root", "d"])
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        assert Config.finetune_all is True and Config.upper_lr == 2e-5 and Config.imu_lr == 1e-5 and Config.imu_dropout == 0.25
        assert Config.clip_grad_norm == float("inf")
        # (the two single options stay what the command line said: the trainer derives its step from finetune_all)
        assert Config.finetune_imu is False and Config.finetune_upper is False
        # the bare form, and the flag off again
        args = p.parse_args(BASE)
        cli.check_finetune(p, args, 1)
        args = p.parse_args(["--train", "--network", "Lower_Net"])
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        assert {k: getattr(Config, k, None) for k in KEYS} == off
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


def test_finetune_all_refusals(capsys, monkeypatch):
    for argv in (["--train", "--network", "Upper_Net", "--finetune_all"], ["--train", "--network", "IMU_Net", "--finetune_all"],
                 ["--train", "--finetune_all"], ["--infer", "--finetune_all"], BASE + ["--infer"], ["--network", "Lower_Net", "--finetune_all"]):
        err = _refused(argv, capsys, monkeypatch)
        assert "--finetune_all" in err and "Lower_Net only" in err, (argv, err)
    err = _refused(BASE + ["--gt_head_pose"], capsys, monkeypatch)
    assert "--finetune_all" in err and "--gt_head_pose" in err
    err = _refused(BASE, capsys, monkeypatch, world=2)
    assert "--finetune_all" in err and "not data parallel" in err
    err = _refused(BASE + ["--resume", "somewhere/epoch0.pth"], capsys, monkeypatch)
    assert "--finetune_all" in err and "--resume" in err
    for other in ("--finetune_imu", "--finetune_upper"):
        err = _refused(BASE + [other], capsys, monkeypatch)
        assert "--finetune_all" in err and "alone" in err, (other, err)
    # the single options' own refusals stand beside it
    err = _refused(["--train", "--network", "Lower_Net", "--finetune_imu"], capsys, monkeypatch)
    assert "Upper_Net only" in err
    err = _refused(["--train", "--network", "Lower_Net", "--imu_lr", "1e-5"], capsys, monkeypatch)
    assert "--imu_lr" in err
    err = _refused(["--train", "--network", "Lower_Net", "--imu_dropout", "0.1"], capsys, monkeypatch)
    assert "--imu_dropout" in err


def test_head_fk_backward_extra_is_declared_and_defined():
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_head_fk_backward_extra"]] == [
        "stream", "which", "y", "body", "B", "F", "dj", "dy", "Rw", "joints_h", "dRw", "dtw", "dR_add", "dt_add"]
    root = os.path.join(os.path.dirname(hip.HEADER), "..", "mmego_amd")
    geom = open(os.path.join(root, "csrc", "geom.hip")).read()
    assert 'extern "C" int mmego_head_fk_backward_extra(' in geom
    sig, _, rest = geom.split("void head_fk_bwd_extra_kernel(")[1].partition(") {\n")
    body = rest.split("\n}\n")[0]
    assert "dR_add" in sig and "rot6d_bwd" in body and "dR_add[" in body
    assert "atomic" not in body and "atomic" not in sig
    # the step's call site passes as many arguments as the prototype has behind the stream
    nets_src = open(os.path.join(root, "nets.py")).read()
    assert nets_src.count('hip.call("head_fk_backward_extra"') == 1
