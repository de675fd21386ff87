"""CPU: the command line's handling of --weight_decay / --decay_mode / --no_decay_1d (a training run's options; the last two shape the first;
everything else is refused with exit code 2 and the flag's name before any work starts), their way into the config and the trainers'
optimiser arguments, the host builder of the decay mask (params.decay_mask_words), FusedAdam's decoupled / no_decay through a saved state,
and the declaration of mmego_adam_step_decay."""
import ctypes
import types

import numpy as np
import pytest
import torch

import main as cli
from decay_helpers import masks, pack_bits
from mmego_amd import hip
from mmego_amd.params import ALIGN, FlatParams, FusedAdam, decay_mask_words, resolve_no_decay

STAGE1 = ["--train", "--network", "IMU_Net"]
STAGE2 = ["--train", "--network", "Upper_Net"]
FLAGS = ("weight_decay", "decay_mode", "no_decay_1d")


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("opts", [["--weight_decay", "0.01"], ["--weight_decay", "0.01", "--decay_mode", "adamw"],
                                  ["--weight_decay", "0.01", "--no_decay_1d"], ["--decay_mode", "l2"], ["--no_decay_1d"]])
def test_decay_options_are_refused_without_a_training_run(capsys, monkeypatch, opts):
    for base in (["--infer"], [], ["--train", "--infer", "--network", "Upper_Net"]):
        err = _refused(base + opts, capsys, monkeypatch)
        assert opts[0] + " goes with --train only" in err, err


def test_mode_and_mask_need_a_decay(capsys, monkeypatch):
    for base in (STAGE1, STAGE2, ["--train", "--network", "Lower_Net", "--finetune_all"]):
        assert "--decay_mode shapes --weight_decay" in _refused(base + ["--decay_mode", "adamw"], capsys, monkeypatch)
        assert "--decay_mode shapes --weight_decay" in _refused(base + ["--decay_mode", "l2", "--no_decay_1d"], capsys, monkeypatch)
        assert "--no_decay_1d shapes --weight_decay" in _refused(base + ["--no_decay_1d"], capsys, monkeypatch)
        assert "--decay_mode" in _refused(base + ["--weight_decay", "0.01", "--decay_mode", "decoupled"], capsys, monkeypatch)


@pytest.mark.parametrize("value", ["-0.01", "-1", "nan", "inf", "-inf"])
def test_a_decay_outside_its_range_is_refused(capsys, monkeypatch, value):
    for base in (STAGE1, STAGE2):
        err = _refused(base + ["--weight_decay=" + value, "--decay_mode", "adamw"], capsys, monkeypatch)
        assert "--weight_decay" in err and "finite and >= 0" in err, err


def test_accepted_forms_reach_the_config_and_the_optimiser_arguments():
    from mmego_amd import processors
    from mmego_amd.config import Config
    p = cli.build_parser()
    names = FLAGS + ("finetune_imu", "imu_lr", "finetune_upper", "upper_lr", "finetune_all", "clip_grad_norm", "ema_decay", "lr_schedule",
                     "lr_warmup", "lr_min_ratio", "lr_decay_steps", "lr_step_every", "lr_step_gamma", "resume_path", "upper_variant", "seed",
                     "window_jitter", "point_keep", "imu_dropout")
    keep = {k: getattr(Config, k, None) for k in names}
    assert (Config.weight_decay, Config.decay_mode, Config.no_decay_1d) == (None, None, False)          # (the defaults: the reference's decays)
    forms = [
        (["--weight_decay", "0.01"], (0.01, None, False), (0.01, False, None)),
        (["--weight_decay", "0"], (0.0, None, False), (0.0, False, None)),
        (["--weight_decay", "0.01", "--decay_mode", "l2"], (0.01, "l2", False), (0.01, False, None)),
        (["--weight_decay", "0.05", "--decay_mode", "adamw"], (0.05, "adamw", False), (0.05, True, None)),
        (["--weight_decay", "0.01", "--no_decay_1d"], (0.01, None, True), (0.01, False, "1d")),
        (["--weight_decay", "0.01", "--decay_mode", "adamw", "--no_decay_1d"], (0.01, "adamw", True), (0.01, True, "1d")),
    ]
    try:
        for base in (STAGE1, STAGE2, STAGE2 + ["--finetune_imu"], ["--train", "--network", "Lower_Net", "--finetune_all"],
                     ["--train", "--network", "Lower_Net", "--finetune_upper"], STAGE2 + ["--upper_variant", "wlocal"],
                     STAGE2 + ["--resume", "x.pth"], STAGE2 + ["--ema_decay", "0.9", "--clip_grad_norm", "1", "--lr_schedule", "cosine"]):
            for opts, want, optimiser in forms:
                args = p.parse_args(base + opts)
                cli.check_finetune(p, args, 1)
                cli.apply_overrides(args)
                assert tuple(getattr(Config, k) for k in FLAGS) == want, (base, opts)
                assert processors._Base._decay_options(types.SimpleNamespace(cfg=Config)) == optimiser
            args = p.parse_args(base)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert tuple(getattr(Config, k) for k in FLAGS) == (None, None, False)
            assert processors._Base._decay_options(types.SimpleNamespace(cfg=Config)) == (None, False, None)
        args = p.parse_args(STAGE1 + ["--weight_decay", "0.01", "--decay_mode", "adamw", "--no_decay_1d"])     # (data parallel: nothing to refuse)
        cli.check_finetune(p, args, 8)
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


def test_the_engines_take_the_options():
    import inspect
    from mmego_amd.train_step import ImuStep, StageStep
    for cls in (StageStep, ImuStep):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["decoupled"].default is False and sig["no_decay"].default is None


# ---- the mask builder ----------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 63, 64, 65, 257)


def _layout(sizes):
    out, off = [], 0
    for i, k in enumerate(sizes):
        out.append(("t%d" % i, off, k))
        off += (k + ALIGN - 1) // ALIGN * ALIGN
    return out, off


def test_mask_bits_against_a_hand_written_layout():
    layout, total = _layout(SIZES)
    assert [o for _, o, _ in layout] == [0, 4, 8, 12, 76, 140, 208] and total == 468        # float4: 1, 1, 1, 16, 16, 17, 65 = 117
    n4 = total // 4
    every = decay_mask_words(layout)
    assert every.dtype == np.uint64 and every.tolist() == [2 ** 64 - 1, 2 ** 53 - 1]         # (bits beyond n4 = 117 are clear)
    assert decay_mask_words(layout, [n for n, _, _ in layout]).tolist() == [0, 0]
    # float4 index ranges by hand: t0 [0,1) t1 [1,2) t2 [2,3) t3 [3,19) t4 [19,35) t5 [35,52) t6 [52,117)
    ranges = {"t0": (0, 1), "t1": (1, 2), "t2": (2, 3), "t3": (3, 19), "t4": (19, 35), "t5": (35, 52), "t6": (52, 117)}
    assert decay_mask_words(layout, {"t1", "t5"}).tolist() == [0xfff00007fffffffd, 0x1fffffffffffff]
    assert decay_mask_words(layout, {"t6"}).tolist() == [2 ** 52 - 1, 0]
    for r in range(1, len(SIZES) + 1):
        for drop in ({"t%d" % i for i in range(len(SIZES)) if (i + r) % 3 == 0}, {"t%d" % (r - 1)}):
            bits = [not any(lo <= i < hi for n, (lo, hi) in ranges.items() if n in drop) for i in range(n4)]
            assert decay_mask_words(layout, drop).tolist() == pack_bits(bits).tolist(), drop
    with pytest.raises(ValueError, match="no_decay names parameters this net does not have: nope"):
        decay_mask_words(layout, {"t1", "nope"})
    assert decay_mask_words([("a", 0, 256)]).tolist() == [2 ** 64 - 1] and decay_mask_words([("a", 0, 260)]).tolist() == [2 ** 64 - 1, 1]
    # (the numpy packing the GPU tests use for their largest mask, against the plain one)
    bits = masks(257)["runs"]
    padded = np.zeros(320, dtype=np.uint8)
    padded[:257] = bits
    assert np.packbits(padded, bitorder="little").view("<u8").tolist() == pack_bits(bits).tolist()
    assert [len(pack_bits(masks(n4)["runs"])) for n4 in (1, 257)] == [1, 5] and pack_bits(masks(257)["last"]).tolist() == [0, 0, 0, 0, 1]


def test_1d_on_the_real_nets():
    from mmego_amd import nets, nets_local
    for net in (nets.UpperNet(), nets.LowerNet(64), nets.IMUNet(15, 9, 32, 2, True, 0), nets_local.UpperNetwlocal()):
        named = dict(net.named_parameters())
        one_d = resolve_no_decay(net, "1d")
        assert list(one_d) == sorted(k for k, p in named.items() if p.dim() <= 1) and 0 < len(one_d) < len(named)
        assert all(k.endswith("bias") or "bias" in k or named[k].dim() == 1 for k in one_d)
        opt = FusedAdam(FlatParams(net), no_decay="1d")
        opt._ensure()
        words = opt._mask.numpy().view(np.uint64)
        layout = opt.layout()
        n4 = opt.flat.flat_p.numel() // 4
        assert len(words) == (n4 + 63) // 64
        want = sum((k + ALIGN - 1) // ALIGN for n, _, k in layout if n not in one_d)
        assert sum(bin(int(w)).count("1") for w in words) == want
        for n, off, k in layout:                                             # first and last float4 of every tensor
            for i in (off // 4, (off + k - 1) // 4):
                assert bool(int(words[i // 64]) >> (i % 64) & 1) == (n not in one_d), n
        tensors, elements = opt.decay_counts()
        dead = {id(q) for q in getattr(net, "never_trained", lambda: ())()}
        assert tensors == len([k for k, q in named.items() if k not in one_d and id(q) not in dead])
        assert elements == sum(q.numel() for k, q in named.items() if k not in one_d and id(q) not in dead)
    with pytest.raises(ValueError, match="does not have: fc9.weight"):
        FusedAdam(FlatParams(torch.nn.Linear(3, 2)), no_decay=["bias", "fc9.weight"])
    with pytest.raises(ValueError, match="no_decay"):
        FusedAdam(FlatParams(torch.nn.Linear(3, 2)), no_decay="2d")
    with pytest.raises(ValueError, match="decoupled"):
        FusedAdam(FlatParams(torch.nn.Linear(3, 2)), decoupled="adamw")
    assert FusedAdam(FlatParams(torch.nn.Linear(3, 2)), no_decay=["bias"]).no_decay == ("bias",)
    assert FusedAdam(FlatParams(torch.nn.Linear(3, 2)), no_decay=[]).no_decay == ()


# ---- the optimiser state ---------------------------------------------------------------------------------------------------------------------------
def test_fused_adam_state_carries_the_decay():
    default = sorted(["m", "v", "state", "lr", "betas", "eps", "weight_decay", "layout", "max_grad_norm"])
    off = FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr=1e-3, weight_decay=1e-2)
    assert sorted(off.state_dict()) == default and off._mask is None and not off.decoupled and off.no_decay == ()
    assert sorted(FusedAdam(FlatParams(torch.nn.Linear(3, 2)), decoupled=False, no_decay=None).state_dict()) == default
    opt = FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr=1e-3, weight_decay=1e-2, decoupled=True, no_decay="1d")
    sd = opt.state_dict()
    assert sorted(sd) == sorted(default + ["decoupled", "no_decay"]) and sd["decoupled"] is True and sd["no_decay"] == ["bias"]
    assert opt._mask.dtype == torch.int64 and opt._mask.tolist() == [0b011]       # weight: 6 floats, two float4; bias: the third
    assert sorted(FusedAdam(FlatParams(torch.nn.Linear(3, 2)), no_decay=["weight"]).state_dict()) == sorted(default + ["no_decay"])
    assert sorted(FusedAdam(FlatParams(torch.nn.Linear(3, 2)), decoupled=True).state_dict()) == sorted(default + ["decoupled"])
    twin = FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr=5.0)                  # (the saved values win, as lr does)
    twin.load_state_dict(sd)
    assert twin.decoupled and twin.no_decay == ("bias",) and twin._mask.tolist() == [0b011] and twin.weight_decay == 1e-2 and twin.lr == 1e-3
    same = FusedAdam(FlatParams(torch.nn.Linear(3, 2)), decoupled=True, no_decay=["bias"])
    same.load_state_dict(sd)
    back = FusedAdam(FlatParams(torch.nn.Linear(3, 2)))                          # (a state without the keys is coupled, all-decay)
    back.load_state_dict(off.state_dict())
    assert not back.decoupled and back.no_decay == () and back._mask is None
    for other, state in ((FusedAdam(FlatParams(torch.nn.Linear(3, 2)), decoupled=True), sd), (FusedAdam(FlatParams(torch.nn.Linear(3, 2)), no_decay="1d"), sd),
                         (opt, off.state_dict())):
        with pytest.raises(ValueError) as e:
            other.load_state_dict(state)
        assert "saved under the weight decay [" in str(e.value) and "this optimiser was built with [" in str(e.value)
        assert "adamw (decoupled), no decay for 1 tensors (bias)" in str(e.value)


def test_the_entry_point_is_declared():
    protos = hip.parse_header()
    names = [n for _, n in protos["mmego_adam_step_sched"]]
    assert [n for _, n in protos["mmego_adam_step_decay"]] == names + ["decay_mask", "decoupled"]
    assert [t for t, _ in protos["mmego_adam_step_decay"]] == [t for t, _ in protos["mmego_adam_step_sched"]] + [ctypes.c_void_p, ctypes.c_int]
    import os
    with open(os.path.join(os.path.dirname(hip.HEADER), "..", "mmego_amd", "csrc", "optim.hip")) as fh:
        assert "mmego_adam_step_decay(" in fh.read()
