"""CPU: the command line's handling of --clip_grad_norm -- a positive threshold (inf allowed) for any training run; everything else is
refused with a message before any work starts -- the declarations of the three entry points behind it, and what FusedAdam's saved state
says about the threshold."""
import math

import pytest
import torch

import main as cli
from mmego_amd import hip

STAGES = [["--train", "--network", n] for n in ("IMU_Net", "Upper_Net", "Lower_Net")]
FINETUNE_IMU = ["--train", "--network", "Upper_Net", "--finetune_imu"]
FINETUNE_UPPER = ["--train", "--network", "Lower_Net", "--finetune_upper"]
KEEP = ("finetune_imu", "imu_lr", "imu_dropout", "resume_path", "finetune_upper", "upper_lr", "clip_grad_norm")


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_clip_grad_norm_reaches_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    keep = {k: getattr(Config, k, None) for k in KEEP}
    assert Config.clip_grad_norm is None                                      # (the default: every optimiser steps as before)
    try:
        for base in STAGES + [FINETUNE_IMU, FINETUNE_UPPER]:
            for text, want in (("2.5", 2.5), ("inf", math.inf), ("1e-3", 1e-3)):
                args = p.parse_args(base + ["--clip_grad_norm", text])
                cli.check_finetune(p, args, 1)
                cli.apply_overrides(args)
                assert Config.clip_grad_norm == want, (base, text)
            args = p.parse_args(base)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.clip_grad_norm is None
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)
    assert Config.clip_grad_norm is None


@pytest.mark.parametrize("value", ["0", "0.0", "-1", "-inf", "nan"])
def test_a_threshold_that_is_not_positive_is_refused(capsys, monkeypatch, value):
    for base in STAGES:
        err = _refused(base + ["--clip_grad_norm=" + value], capsys, monkeypatch)
        assert "--clip_grad_norm is a gradient-norm threshold" in err and "> 0" in err, err


def test_clip_grad_norm_is_refused_outside_training(capsys, monkeypatch):
    for argv in (["--infer", "--clip_grad_norm", "1"], ["--clip_grad_norm", "1"], ["--network", "IMU_Net", "--clip_grad_norm", "1"],
                 ["--infer", "--train", "--network", "IMU_Net", "--clip_grad_norm", "1"]):
        err = _refused(argv, capsys, monkeypatch)
        assert "--clip_grad_norm goes with --train only" in err, err


def test_clipping_entry_points_are_declared():
    """The three new entry points are in the header, with the argument lists FusedAdam passes (hip.py binds from the header); the plain
    step's declaration is what it was."""
    protos = hip.parse_header()
    adam = ["stream", "p", "g", "m", "v", "n", "state", "lr", "beta1", "beta2", "eps", "weight_decay", "skip", "nskip", "ticket"]
    assert [n for _, n in protos["mmego_adam_step"]] == adam
    assert [n for _, n in protos["mmego_grad_norm_nblk"]] == ["n"]
    assert [n for _, n in protos["mmego_grad_sqnorm"]] == ["stream", "g", "n", "skip", "nskip", "part", "npart"]
    assert [n for _, n in protos["mmego_adam_step_clipped"]] == adam + ["part", "npart", "max_norm", "stats"]


def test_record_count_is_a_function_of_n_alone():
    nblk = hip.lib().mmego_grad_norm_nblk                                     # (pure host helper: safe without a GPU)
    assert [nblk(n) for n in (4, 1024, 1028, 4104)] == [1, 1, 2, 5]
    assert max(nblk(n) for n in (1 << 20, 1 << 24, 1 << 31, 1 << 40)) <= 2048
    assert nblk(1 << 24) == nblk(1 << 24)


def _opt(max_grad_norm=None):
    from mmego_amd.params import FlatParams, FusedAdam
    torch.manual_seed(0)
    return FusedAdam(FlatParams(torch.nn.Linear(3, 5)), lr=1e-3, max_grad_norm=max_grad_norm)


def test_fused_adam_state_carries_the_threshold():
    a = _opt(2.5)
    sd = a.state_dict()
    assert sd["max_grad_norm"] == 2.5
    assert set(sd) == {"m", "v", "state", "lr", "betas", "eps", "weight_decay", "layout", "max_grad_norm"}    # (no statistics in it)
    b = _opt()                                                                # (a resumed run that does not repeat the flag)
    assert b.max_grad_norm is None and b.state_dict()["max_grad_norm"] is None
    b.load_state_dict(sd)
    assert b.max_grad_norm == 2.5 and b.state_dict()["max_grad_norm"] == 2.5
    c = _opt(2.5)
    c.load_state_dict(_opt().state_dict())                                    # (the saved run did not clip: neither does its continuation)
    assert c.max_grad_norm is None
    old = {k: v for k, v in sd.items() if k != "max_grad_norm"}               # (a state written before the key existed)
    for start in (None, 4.0):
        d = _opt(start)
        d.load_state_dict(old)
        assert d.max_grad_norm == start
    with pytest.raises(ValueError, match="max_grad_norm"):
        _opt(-1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        _opt(float("nan"))
    assert _opt(float("inf")).max_grad_norm == math.inf
