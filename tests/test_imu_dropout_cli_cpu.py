"""CPU: the command line's handling of --imu_dropout -- it belongs to the two runs that train an IMU_Net (stage 1, --finetune_imu) and
takes a rate in [0, 1); everything else is refused with a message before any work starts -- and the declarations of the two entry
points behind it."""
import pytest

import main as cli
from mmego_amd import hip

STAGE1 = ["--train", "--network", "IMU_Net"]
FINETUNE = ["--train", "--network", "Upper_Net", "--finetune_imu"]


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_imu_dropout_is_refused_where_no_imu_net_is_trained(capsys, monkeypatch):
    for argv in (["--infer", "--imu_dropout", "0.1"],
                 ["--train", "--network", "Lower_Net", "--imu_dropout", "0.1"],
                 ["--train", "--network", "Upper_Net", "--imu_dropout", "0.1"]):
        err = _refused(argv, capsys, monkeypatch)
        assert "--imu_dropout goes with" in err and "--finetune_imu" in err, err


@pytest.mark.parametrize("value", ["-0.1", "1.0", "1.5"])
def test_imu_dropout_rate_outside_the_unit_interval_is_refused(capsys, monkeypatch, value):
    for base in (STAGE1, FINETUNE):
        assert "[0, 1)" in _refused(base + ["--imu_dropout=" + value], capsys, monkeypatch)


def test_imu_dropout_reaches_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    keep = {k: getattr(Config, k, None) for k in ("finetune_imu", "imu_lr", "imu_dropout", "resume_path", "finetune_upper", "upper_lr")}
    assert Config.imu_dropout is None                                       # (the default: every net is built as before)
    try:
        for base in (STAGE1, FINETUNE):
            args = p.parse_args(base + ["--imu_dropout", "0.1"])
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.imu_dropout == 0.1 and Config.finetune_imu is (base is FINETUNE)
            args = p.parse_args(base)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.imu_dropout is None
        args = p.parse_args(STAGE1 + ["--imu_dropout", "0"])                # (0 is a rate too)
        cli.check_finetune(p, args, 1)
        cli.apply_overrides(args)
        assert Config.imu_dropout == 0.0
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


def test_dropout_entry_points_are_declared():
    """The two new entry points are in the header, with the argument lists ops.py passes (hip.py binds from the header)."""
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_seed_take"]] == ["stream", "seed_ctr", "taken"]
    assert [n for _, n in protos["mmego_lstm_dropout"]] == ["stream", "X", "ldx", "Y", "ldy", "rows", "cols", "p", "seed_word", "salt"]
