"""CPU: the command line's handling of --finetune_upper / --upper_lr -- every arrangement the mode does not support is refused with a
message before any work starts -- and the C ABI of the Lower_Net input-gradient kernels."""
import os
import re

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


def test_finetune_upper_argument_handling(capsys, monkeypatch):
    base = ["--train", "--network", "Lower_Net", "--finetune_upper"]
    assert "Lower_Net only" in _refused(["--train", "--network", "Upper_Net", "--finetune_upper"], capsys, monkeypatch)
    assert "Lower_Net only" in _refused(["--train", "--network", "IMU_Net", "--finetune_upper"], capsys, monkeypatch)
    assert "Lower_Net only" in _refused(["--infer", "--finetune_upper"], capsys, monkeypatch)
    assert "Lower_Net only" in _refused(base + ["--infer"], capsys, monkeypatch)
    err = _refused(base, capsys, monkeypatch, world=2)
    assert "--finetune_upper" in err and "not data parallel" in err
    err = _refused(base + ["--resume", "somewhere/epoch0.pth"], capsys, monkeypatch)
    assert "--finetune_upper" in err and "--resume" in err
    err = _refused(["--train", "--network", "Lower_Net", "--upper_lr", "1e-5"], capsys, monkeypatch)
    assert "--upper_lr" in err and "--finetune_upper" in err


def test_finetune_upper_accepts_the_recorded_head_pose():
    """--gt_head_pose is allowed (the pose is not what is trained); the checks pass without touching a device."""
    p = cli.build_parser()
    args = p.parse_args(["--train", "--network", "Lower_Net", "--finetune_upper", "--gt_head_pose", "--upper_lr", "1e-5"])
    cli.check_finetune(p, args, 1)


def test_finetune_upper_flags_reach_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    args = p.parse_args(["--train", "--network", "Lower_Net", "--finetune_upper", "--upper_lr", "2e-5"])
    cli.check_finetune(p, args, 1)
    keep = {k: getattr(Config, k, None) for k in ("finetune_upper", "upper_lr", "finetune_imu", "imu_lr", "resume_path")}
    try:
        cli.apply_overrides(args)
        assert Config.finetune_upper is True and Config.upper_lr == 2e-5 and Config.finetune_imu is False
        args = p.parse_args(["--train", "--network", "Lower_Net"])
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        assert Config.finetune_upper is False and Config.upper_lr is None        # (upper_lr None: the step falls back to lr)
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


def test_lower_input_gradient_entry_points_are_declared():
    """The new entry points are in the header (hip.py binds from it) with the argument lists nets.LowerNet passes, and the transform
    backward is a fixed-order reduction."""
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_lower_inputs_backward"]] == [
        "stream", "pts", "ldp", "F", "N", "idx", "P", "R", "t", "g", "ldg", "g2", "ldg2", "joints", "V", "gj", "ldgj", "gj2", "ldgj2",
        "accumulate", "dR", "dt", "djoints"]
    assert [n for _, n in protos["mmego_bn_input_grad"]] == ["stream", "dY", "lddy", "X", "ldx", "state", "rows", "C", "dgamma", "dbeta",
                                                            "dX", "lddx"]
    root = os.path.join(os.path.dirname(hip.HEADER), "..", "mmego_amd")
    geom = open(os.path.join(root, "csrc", "geom.hip")).read()
    assert 'extern "C" int mmego_lower_inputs_backward(' in geom
    assert 'extern "C" int mmego_bn_input_grad(' in open(os.path.join(root, "csrc", "gcn_fused.hip")).read()
    body = geom.split("void lower_inputs_bwd_kernel")[1].split("__global__")[0]
    assert "wave_sum" in body and "atomicAdd" not in body and "atomic" not in body
    # every call site in nets.py passes as many arguments as the prototype has behind the stream
    nets_src = open(os.path.join(root, "nets.py")).read()
    calls = re.findall(r'hip\.call\("lower_inputs_backward",(.*?)\)\n', nets_src, flags=re.S)
    assert len(calls) == 2
    for c in calls:
        depth, n = 0, 1
        for ch in c:
            depth += ch in "([" 
            depth -= ch in ")]"
            n += (ch == "," and depth == 0)
        assert n == len(protos["mmego_lower_inputs_backward"]) - 1, (n, c)
