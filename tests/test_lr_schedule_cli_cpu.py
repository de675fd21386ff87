"""CPU: the command line's handling of the --lr_* options (a training run's options; each belongs to the kinds that read it and has its
range; everything else is refused with exit code 2 and the flag's name before any work starts), the value class params.LrSchedule
(validation as the C side's, dict round trip, multiplier against tests/lr_schedule_ref.py), the default span, the descriptor's layout
against the C compiler's, and the schedule's passage through a saved optimiser state."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

import main as cli
from lr_schedule_ref import default_span, mult_ref
from mmego_amd import hip
from mmego_amd.params import FlatParams, FusedAdam, LrSchedule, lr_schedule_of

STAGE1 = ["--train", "--network", "IMU_Net"]
STAGE2 = ["--train", "--network", "Upper_Net"]
STEP = ["--lr_schedule", "step", "--lr_step_every", "5", "--lr_step_gamma", "0.5"]
FLAGS = ("lr_schedule", "lr_warmup", "lr_min_ratio", "lr_decay_steps", "lr_step_every", "lr_step_gamma")


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("opts", [["--lr_schedule", "cosine"], ["--lr_warmup", "3"], ["--lr_schedule", "linear", "--lr_min_ratio", "0.1"],
                                  ["--lr_schedule", "cosine", "--lr_decay_steps", "10"], STEP])
def test_lr_options_are_refused_without_a_training_run(capsys, monkeypatch, opts):
    for base in (["--infer"], [], ["--train", "--infer", "--network", "Upper_Net"]):
        err = _refused(base + opts, capsys, monkeypatch)
        assert opts[0] + " goes with --train only" in err, err


def test_options_that_belong_to_another_kind_are_refused(capsys, monkeypatch):
    for base in (STAGE1, STAGE2):
        assert "--lr_min_ratio" in _refused(base + ["--lr_min_ratio", "0.1"], capsys, monkeypatch)
        assert "--lr_min_ratio" in _refused(base + ["--lr_warmup", "3", "--lr_min_ratio", "0.1"], capsys, monkeypatch)
        assert "--lr_decay_steps" in _refused(base + ["--lr_decay_steps", "10"], capsys, monkeypatch)
        assert "--lr_decay_steps" in _refused(base + STEP + ["--lr_decay_steps", "10"], capsys, monkeypatch)
        for kind in ([], ["--lr_schedule", "cosine"], ["--lr_schedule", "linear"]):
            assert "--lr_step_every" in _refused(base + kind + ["--lr_step_every", "5"], capsys, monkeypatch)
            assert "--lr_step_gamma" in _refused(base + kind + ["--lr_step_gamma", "0.5"], capsys, monkeypatch)
        err = _refused(base + ["--lr_schedule", "step", "--lr_step_every", "5"], capsys, monkeypatch)
        assert "--lr_schedule step needs" in err and "--lr_step_gamma is missing" in err
        err = _refused(base + ["--lr_schedule", "step", "--lr_step_gamma", "0.5"], capsys, monkeypatch)
        assert "--lr_schedule step needs" in err and "--lr_step_every is missing" in err
        assert "--lr_schedule step needs" in _refused(base + ["--lr_schedule", "step"], capsys, monkeypatch)
        assert "--lr_schedule" in _refused(base + ["--lr_schedule", "exponential"], capsys, monkeypatch)


@pytest.mark.parametrize("flag,values,kind", [
    ("--lr_warmup", ["0", "-1", "1.5", "nan", "inf"], []),
    ("--lr_min_ratio", ["1", "1.0", "-0.1", "1.5", "nan", "inf"], ["--lr_schedule", "cosine"]),
    ("--lr_decay_steps", ["0", "-3", "2.5", "nan", "inf"], ["--lr_schedule", "linear"]),
    ("--lr_step_every", ["0", "-1", "0.5", "nan", "inf"], ["--lr_schedule", "step", "--lr_step_gamma", "0.5"]),
    ("--lr_step_gamma", ["0", "0.0", "-0.5", "1.01", "nan", "inf"], ["--lr_schedule", "step", "--lr_step_every", "5"]),
])
def test_values_outside_their_ranges_are_refused(capsys, monkeypatch, flag, values, kind):
    for value in values:
        err = _refused(STAGE2 + kind + [flag + "=" + value], capsys, monkeypatch)
        assert flag in err, (value, err)


def test_accepted_forms_reach_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    names = FLAGS + ("finetune_imu", "imu_lr", "imu_dropout", "resume_path", "finetune_upper", "upper_lr", "finetune_all", "clip_grad_norm",
                     "ema_decay", "window_jitter", "point_keep", "seed")
    keep = {k: getattr(Config, k, None) for k in names}
    assert all(getattr(Config, k) is None for k in FLAGS)                   # (the defaults: a constant rate everywhere)
    forms = [
        (["--lr_schedule", "cosine"], ("cosine", None, None, None, None, None)),
        (["--lr_warmup", "100"], (None, 100, None, None, None, None)),
        (["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_decay_steps", "7", "--lr_min_ratio", "0.1"], ("cosine", 2, 0.1, 7, None, None)),
        (["--lr_schedule", "linear", "--lr_min_ratio", "0"], ("linear", None, 0.0, None, None, None)),
        (STEP + ["--lr_warmup", "1", "--lr_min_ratio", "0.2"], ("step", 1, 0.2, None, 5, 0.5)),
        (["--lr_schedule", "step", "--lr_step_every", "1", "--lr_step_gamma", "1"], ("step", None, None, None, 1, 1.0)),
    ]
    try:
        for base in (STAGE1, STAGE2, STAGE2 + ["--finetune_imu"], ["--train", "--network", "Lower_Net", "--finetune_all"],
                     STAGE2 + ["--ema_decay", "0.9", "--clip_grad_norm", "1"]):
            for opts, want in forms:
                args = p.parse_args(base + opts)
                cli.check_finetune(p, args, 1)
                cli.apply_overrides(args)
                assert tuple(getattr(Config, k) for k in FLAGS) == want, (base, opts)
            args = p.parse_args(base)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert all(getattr(Config, k) is None for k in FLAGS)
            assert lr_schedule_of(Config, 10, 5) is None
        args = p.parse_args(STAGE1 + ["--lr_schedule", "cosine", "--lr_warmup", "5"])     # (data parallel: nothing to refuse)
        cli.check_finetune(p, args, 8)
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


class _Cfg:
    def __init__(self, **kw):
        for k in FLAGS:
            setattr(self, k, kw.get(k))


def test_the_schedule_of_a_config_and_its_default_span():
    assert lr_schedule_of(_Cfg(), 10, 7) is None
    s = lr_schedule_of(_Cfg(lr_warmup=4), 10, 7)
    assert s == LrSchedule("constant", warmup=4) and s.span is None
    for kind in ("cosine", "linear"):
        for epochs, per_epoch, warmup in ((10, 7, 4), (2, 3, 0), (1, 2, 5), (1, 5, 5), (3, 1, 2)):
            s = lr_schedule_of(_Cfg(lr_schedule=kind, lr_warmup=warmup or None, lr_min_ratio=0.25), epochs, per_epoch)
            assert s.span == default_span(epochs, per_epoch, warmup) >= 1 and s.warmup == warmup and s.floor == 0.25 and s.kind == kind
        s = lr_schedule_of(_Cfg(lr_schedule=kind, lr_decay_steps=13), 10, 7)        # (--lr_decay_steps overrides)
        assert s.span == 13 and s.floor == 0.0 and s.warmup == 0
    s = lr_schedule_of(_Cfg(lr_schedule="step", lr_step_every=5, lr_step_gamma=0.5, lr_min_ratio=0.2, lr_warmup=1), 10, 7)
    assert s == LrSchedule("step", warmup=1, floor=0.2, every=5, gamma=0.5)


NAN, INF = float("nan"), float("inf")
BAD = [dict(kind="exponential"), dict(kind=1), dict(warmup=-1), dict(warmup=1.5), dict(warmup=NAN), dict(warmup=INF),
       dict(floor=1.0), dict(floor=-0.1), dict(floor=NAN), dict(floor=INF),
       dict(kind="cosine"), dict(kind="cosine", span=0), dict(kind="linear", span=2.5), dict(kind="cosine", span=NAN), dict(kind="linear", span=INF),
       dict(kind="constant", span=3), dict(kind="step", every=2, gamma=0.5, span=3),
       dict(kind="step", gamma=0.5), dict(kind="step", every=0, gamma=0.5), dict(kind="step", every=1.5, gamma=0.5),
       dict(kind="step", every=NAN, gamma=0.5), dict(kind="step", every=INF, gamma=0.5),
       dict(kind="step", every=2), dict(kind="step", every=2, gamma=0.0), dict(kind="step", every=2, gamma=1.5), dict(kind="step", every=2, gamma=NAN),
       dict(kind="cosine", span=3, every=2), dict(kind="constant", gamma=0.5)]


@pytest.mark.parametrize("kw", BAD, ids=[str(i) for i in range(len(BAD))])
def test_lr_schedule_refuses_what_the_c_side_refuses(kw):
    with pytest.raises(ValueError, match="LrSchedule"):
        LrSchedule(**kw)


GOOD = [dict(), dict(warmup=3), dict(kind="cosine", warmup=3, span=3, floor=0.1), dict(kind="cosine", span=1), dict(kind="linear", warmup=3, span=3),
        dict(kind="linear", span=4, floor=0.3), dict(kind="step", warmup=3, every=2, gamma=0.5, floor=0.2), dict(kind="step", every=1, gamma=1.0)]


@pytest.mark.parametrize("kw", GOOD, ids=[str(i) for i in range(len(GOOD))])
def test_lr_schedule_round_trip_struct_and_multiplier(kw):
    s = LrSchedule(**kw)
    d = s.to_dict()
    assert set(d) == set(LrSchedule.FIELDS) and LrSchedule.from_dict(d) == s and hash(LrSchedule.from_dict(d)) == hash(s)
    assert LrSchedule.from_dict(dict(d, warmup=s.warmup + 1)) != s
    c = s.c_struct()
    assert isinstance(c, hip.LrSchedule) and c.kind == LrSchedule.KINDS.index(s.kind) and c.reserved == 0 and c.warmup == s.warmup
    assert c.floor == s.floor and (s.span is None or c.span == s.span) and (s.every is None or (c.every, c.gamma) == (s.every, s.gamma))
    worst = 0.0
    for t in range(1, 12):
        want = mult_ref(s.kind, t, W=s.warmup, D=s.span or 1, r=s.floor, E=s.every or 1, g=s.gamma or 1.0)
        got = s.multiplier(t)
        assert abs(got - want) <= 4 * 2.0 ** -53, (t, got, want)           # (the same few float64 operations, grouped alike or not)
        worst = max(worst, abs(got - want))
        if t <= s.warmup:                                                   # exactly 1 (times the warm-up factor) where s == 0
            assert got == (t / s.warmup if t < s.warmup else 1.0), t
    if s.warmup:
        assert s.multiplier(s.warmup) == 1.0 and s.multiplier(1) == 1.0 / s.warmup
    if s.kind in ("cosine", "linear"):
        end = s.multiplier(s.warmup + s.span)
        assert abs(end - s.floor) <= 2.0 ** -52 and s.multiplier(s.warmup + s.span + 50) == end       # (holds past the span)
    print("%r: worst |multiplier - reference| = %.3g" % (s, worst))


def test_the_reference_multiplier_itself():
    """The definition's landmarks, by hand: W = 3, D = 3."""
    assert [mult_ref("constant", t, W=3) for t in (1, 2, 3, 4, 9)] == [1 / 3, 2 / 3, 1.0, 1.0, 1.0]
    assert mult_ref("cosine", 3, W=3, D=3, r=0.1) == 1.0 and mult_ref("linear", 3, W=3, D=3, r=0.1) == 1.0
    assert abs(mult_ref("cosine", 6, W=3, D=3, r=0.1) - 0.1) < 1e-15 and mult_ref("cosine", 7, W=3, D=3, r=0.1) == mult_ref("cosine", 6, W=3, D=3, r=0.1)
    assert abs(mult_ref("linear", 4, W=3, D=3, r=0.1) - (0.1 + 0.9 * 2 / 3)) < 1e-15
    assert abs(mult_ref("cosine", 4, W=3, D=3, r=0.0) - (1 + math.cos(math.pi / 3)) / 2) < 1e-15
    assert [mult_ref("step", t, W=3, r=0.2, E=2, g=0.5) for t in range(3, 11)] == [1.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.2, 0.2]


def test_the_descriptor_matches_the_c_layout(tmp_path):
    """MmegoLrSchedule is declared as a tagged struct with its typedef behind it; hip.parse_tagged_structs mirrors it.  The header is compiled
    with gcc (it is plain C) into a program that prints sizeof and every field's offset: the class must agree field by field."""
    cls = hip.parse_tagged_structs(hip.header_text())["MmegoLrSchedule"]
    assert cls.__name__ == "LrSchedule" and [n for n, _ in cls._fields_] == ["kind", "reserved", "warmup", "span", "floor", "every", "gamma"]
    assert "MmegoLrSchedule" not in hip.parse_structs(hip.header_text())
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % hip.HEADER, "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(MmegoLrSchedule));']
    lines += ['  printf("%s %%zu\\n", offsetof(MmegoLrSchedule, %s));' % (n, n) for n, _ in cls._fields_]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == int(got.pop("sizeof")) == 48
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == {k: int(v) for k, v in got.items()}
    # the reader refuses in this spelling what it refuses in the other
    with pytest.raises(RuntimeError, match="mmego_hip.h"):
        hip.parse_tagged_structs("struct MmegoT { short a; };\ntypedef struct MmegoT MmegoT;")
    assert hip.parse_tagged_structs("struct MmegoT { int a; };") == {}          # (no typedef behind it: not a descriptor)


def test_the_entry_point_is_declared():
    protos = hip.parse_header()
    names = [n for _, n in protos["mmego_adam_step_clipped_ema"]]
    assert [n for _, n in protos["mmego_adam_step_sched"]] == names + ["sched"]
    assert [t for t, _ in protos["mmego_adam_step_sched"]] == [t for t, _ in protos["mmego_adam_step_clipped_ema"]] + [ctypes.c_void_p]
    with open(os.path.join(os.path.dirname(hip.HEADER), "..", "mmego_amd", "csrc", "optim.hip")) as fh:
        src = fh.read()
    for name in ("mmego_adam_step", "mmego_adam_step_clipped", "mmego_adam_step_ema", "mmego_adam_step_clipped_ema", "mmego_adam_step_sched"):
        assert name + "(" in src, name


def test_fused_adam_state_carries_the_schedule():
    """Without a device (no step): the state is set by hand."""
    sched = LrSchedule("cosine", warmup=3, span=3, floor=0.1)
    with pytest.raises(ValueError, match="lr_schedule"):
        FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr_schedule="cosine")
    off = FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr=1e-3)
    off._ensure()
    assert off.state.numel() == 3 and "lr_schedule" not in off.state_dict() and off.current_lr() == 1e-3
    assert sorted(off.state_dict()) == sorted(["m", "v", "state", "lr", "betas", "eps", "weight_decay", "layout", "max_grad_norm"])
    opt = FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr=1e-3, lr_schedule=sched)
    opt._ensure()
    assert opt.state.numel() == 4 and opt.current_lr() == 1e-3 * mult_ref("cosine", 1, W=3, D=3, r=0.1) == 1e-3 * (1.0 / 3.0)
    opt.state.copy_(torch.tensor([5.0, 0.5, 0.25, 3.25e-4], dtype=torch.float64))
    assert opt.current_lr() == 3.25e-4
    sd = opt.state_dict()
    assert sd["lr_schedule"] == sched.to_dict() and sd["state"].numel() == 4
    twin = FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr=5.0, lr_schedule=LrSchedule.from_dict(sd["lr_schedule"]))
    twin.load_state_dict(sd)
    assert torch.equal(twin.state, opt.state) and twin.lr == 1e-3
    # a three-word state into a scheduled optimiser: the schedule takes up at the saved count, state[3] is 0 until its first step
    off.state.copy_(torch.tensor([4.0, 0.5, 0.25], dtype=torch.float64))
    twin.load_state_dict(off.state_dict())
    assert twin.state.tolist() == [4.0, 0.5, 0.25, 0.0] and twin.current_lr() == 1e-3 * mult_ref("cosine", 5, W=3, D=3, r=0.1)
    # a differing saved schedule is refused, and the message names both
    other = LrSchedule("linear", warmup=3, span=3, floor=0.1)
    for dst in (FusedAdam(FlatParams(torch.nn.Linear(3, 2)), lr_schedule=other), FusedAdam(FlatParams(torch.nn.Linear(3, 2)))):
        with pytest.raises(ValueError) as e:
            dst.load_state_dict(sd)
        assert repr(sched) in str(e.value) and repr(dst.lr_schedule) in str(e.value)
