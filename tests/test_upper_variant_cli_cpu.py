"""CPU: the command line's handling of --upper_variant -- its default, every arrangement it does not support refused with a message before
any work starts, the flag's way into the configs, and the check that tells a checkpoint of the other variant by its keys."""
import pytest

import main as cli


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def _config_kept(*classes):
    names = ("upper_variant", "finetune_imu", "imu_lr", "imu_dropout", "finetune_upper", "upper_lr", "finetune_all", "clip_grad_norm", "resume_path")
    return [(c, k, getattr(c, k)) for c in classes for k in names if hasattr(c, k)]


def test_upper_variant_default_is_global():
    from mmego_amd.config import Config, ConfigDemo
    assert Config.upper_variant == "global" and ConfigDemo.upper_variant == "global"
    p = cli.build_parser()
    keep = _config_kept(Config, ConfigDemo)
    try:
        for argv in (["--train", "--network", "Upper_Net"], ["--train", "--network", "Lower_Net"], ["--infer"],
                     ["--train", "--network", "IMU_Net"]):
            args = p.parse_args(argv)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.upper_variant == "global" and ConfigDemo.upper_variant == "global", argv
    finally:
        for c, k, v in keep:
            setattr(c, k, v)
    with pytest.raises(SystemExit):
        p.parse_args(["--train", "--network", "Upper_Net", "--upper_variant", "voxel"])       # (a choice, not free text)


def test_upper_variant_refusals(capsys, monkeypatch):
    for v in ("global", "wlocal"):
        err = _refused(["--train", "--network", "IMU_Net", "--upper_variant", v], capsys, monkeypatch)
        assert "--upper_variant" in err and "IMU_Net" in err
    err = _refused(["--train", "--network", "Lower_Net", "--upper_variant", "wlocal", "--finetune_upper"], capsys, monkeypatch)
    assert "--upper_variant wlocal" in err and "--finetune_upper" in err
    err = _refused(["--train", "--network", "Lower_Net", "--upper_variant", "wlocal", "--finetune_all"], capsys, monkeypatch)
    assert "--upper_variant wlocal" in err and "--finetune_all" in err
    # global with the same options is what it was: accepted by the checks
    p = cli.build_parser()
    for flag in ("--finetune_upper", "--finetune_all"):
        cli.check_finetune(p, p.parse_args(["--train", "--network", "Lower_Net", "--upper_variant", "global", flag]), 1)
    # everything --train --network Upper_Net composes with for global composes with wlocal
    for extra in (["--finetune_imu", "--imu_lr", "1e-5", "--imu_dropout", "0.1"], ["--clip_grad_norm", "1.0"], ["--resume", "somewhere/epoch0.pth"],
                  ["--gt_head_pose"]):
        cli.check_finetune(p, p.parse_args(["--train", "--network", "Upper_Net", "--upper_variant", "wlocal"] + extra), 1)
    cli.check_finetune(p, p.parse_args(["--infer", "--upper_variant", "wlocal"]), 1)
    cli.check_finetune(p, p.parse_args(["--train", "--network", "Lower_Net", "--upper_variant", "wlocal"]), 1)


def test_upper_variant_reaches_the_configs():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    keep = _config_kept(Config, ConfigDemo)
    try:
        args = p.parse_args(["--train", "--network", "Upper_Net", "--upper_variant", "wlocal", "--finetune_imu"])
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        assert Config.upper_variant == "wlocal" and ConfigDemo.upper_variant == "wlocal" and Config.finetune_imu is True
        args = p.parse_args(["--infer"])
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        assert Config.upper_variant == "global" and ConfigDemo.upper_variant == "global"
    finally:
        for c, k, v in keep:
            setattr(c, k, v)


def test_checkpoint_of_the_other_variant_is_refused_by_name():
    """processors.load_upper_state: the message names the flag and both variants; a checkpoint of the right variant loads."""
    import torch
    from mmego_amd import nets, nets_local, processors
    torch.manual_seed(0)
    glob, wloc = nets.UpperNet(), nets_local.UpperNetwlocal()
    assert processors.upper_variant_of(glob.state_dict()) == "global" and processors.upper_variant_of(wloc.state_dict()) == "wlocal"
    assert processors.UPPER_VARIANTS == {"global": nets.UpperNet, "wlocal": nets_local.UpperNetwlocal}
    with pytest.raises(SystemExit) as e:
        processors.load_upper_state(nets_local.UpperNetwlocal(), glob.state_dict(), "wlocal", "some/upper.pth")
    msg = str(e.value)
    assert "--upper_variant global" in msg and "some/upper.pth" in msg and "Missing key" not in msg
    with pytest.raises(SystemExit) as e:
        processors.load_upper_state(nets.UpperNet(), wloc.state_dict(), "global", "some/upper.pth")
    assert "--upper_variant wlocal" in str(e.value)
    other = nets_local.UpperNetwlocal()
    processors.load_upper_state(other, wloc.state_dict(), "wlocal", "some/upper.pth")
    for k, v in wloc.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k


def test_parameter_names_and_flat_order_of_both_upper_nets_are_the_recorded_ones():
    """named_parameters, named_buffers and flat_param_order (as names) of a fresh UpperNet and a fresh UpperNetwlocal equal
    tests/golden/upper_param_order.json, recorded on the commit before the two nets got one base class: checkpoints, upper_variant_of and
    the flat buffer's layout depend on names and registration order."""
    import json
    import os

    from conftest import GOLDEN
    from mmego_amd import nets, nets_local
    want = json.load(open(os.path.join(GOLDEN, "upper_param_order.json")))
    assert sorted(want) == ["UpperNet", "UpperNetwlocal"]
    for cls in (nets.UpperNet, nets_local.UpperNetwlocal):
        net = cls()
        names = {id(p): n for n, p in net.named_parameters()}
        got = {"named_parameters": [n for n, _ in net.named_parameters()], "named_buffers": [n for n, _ in net.named_buffers()],
               "flat_param_order": [names[id(p)] for p in net.flat_param_order()]}
        assert got == want[cls.__name__], cls.__name__
