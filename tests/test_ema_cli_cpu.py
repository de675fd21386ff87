"""CPU: the command line's handling of --ema_decay (a training run's option, a decay strictly inside (0, 1); everything else is refused
with a message before any work starts), FusedAdam's own refusal of bad decays, the declarations of the two entry points behind the
option, and the average's passage through a saved optimiser state -- by name, also when the flat layout changed in between."""
import pytest
import torch

import main as cli
from mmego_amd import hip

STAGE1 = ["--train", "--network", "IMU_Net"]
STAGE2 = ["--train", "--network", "Upper_Net"]


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("value", ["0", "1", "1.0", "-0.1", "1.5", "nan", "inf"])
def test_ema_decay_outside_the_open_unit_interval_is_refused(capsys, monkeypatch, value):
    for base in (STAGE1, STAGE2, ["--train", "--network", "Lower_Net", "--finetune_all"]):
        err = _refused(base + ["--ema_decay=" + value], capsys, monkeypatch)
        assert "--ema_decay is the decay of the weight average" in err and "(0, 1)" in err, err


def test_ema_decay_is_refused_without_a_training_run(capsys, monkeypatch):
    for argv in (["--infer", "--ema_decay", "0.9"], ["--ema_decay", "0.9"], ["--infer", "--dense", "--ema_decay", "0.9"],
                 ["--train", "--infer", "--network", "Upper_Net", "--ema_decay", "0.9"]):
        assert "--ema_decay goes with --train only" in _refused(argv, capsys, monkeypatch)


def test_ema_decay_reaches_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    names = ("finetune_imu", "imu_lr", "imu_dropout", "resume_path", "finetune_upper", "upper_lr", "finetune_all", "clip_grad_norm",
             "ema_decay", "window_jitter", "point_keep", "seed")
    keep = {k: getattr(Config, k, None) for k in names}
    assert Config.ema_decay is None                                         # (the default: no average anywhere)
    try:
        for base in (STAGE1, STAGE2, STAGE2 + ["--finetune_imu"], ["--train", "--network", "Lower_Net", "--finetune_upper"],
                     STAGE2 + ["--upper_variant", "wlocal"], STAGE2 + ["--window_jitter", "--point_keep", "0.8"]):
            args = p.parse_args(base + ["--ema_decay", "0.999"])
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.ema_decay == 0.999
            args = p.parse_args(base)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.ema_decay is None
        args = p.parse_args(STAGE1 + ["--ema_decay", "0.9"])                # (data parallel: nothing to refuse)
        cli.check_finetune(p, args, 8)
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)


@pytest.mark.parametrize("value", [0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")])
def test_fused_adam_refuses_a_decay_outside_the_open_unit_interval(value):
    from mmego_amd.params import FlatParams, FusedAdam
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdam(FlatParams(torch.nn.Linear(3, 2)), ema_decay=value)


def test_fused_adam_without_a_decay_keeps_no_average():
    from mmego_amd.params import FlatParams, FusedAdam
    opt = FusedAdam(FlatParams(torch.nn.Linear(3, 2)))
    opt._ensure()
    assert opt.ema_decay is None and opt.ema is None
    assert "ema" not in opt.state_dict() and "ema_decay" not in opt.state_dict()
    with pytest.raises(RuntimeError, match="no weight average"):
        with opt.averaged():
            pass
    with pytest.raises(RuntimeError, match="no weight average"):
        opt.ema_state_dict()


def test_ema_entry_points_are_declared():
    """The two new entry points are in the header: the argument list of the plain counterpart, then the average and its decay -- what
    params.FusedAdam.step passes (hip.py binds from the header)."""
    protos = hip.parse_header()
    for plain in ("mmego_adam_step", "mmego_adam_step_clipped"):
        names = [n for _, n in protos[plain]]
        assert [n for _, n in protos[plain + "_ema"]] == names + ["ema", "ema_decay"]
        import ctypes
        assert [t for t, _ in protos[plain + "_ema"]] == [t for t, _ in protos[plain]] + [ctypes.c_void_p, ctypes.c_double]
    assert [n for _, n in protos["mmego_adam_step_ema"]] == ["stream", "p", "g", "m", "v", "n", "state", "lr", "beta1", "beta2", "eps",
                                                             "weight_decay", "skip", "nskip", "ticket", "ema", "ema_decay"]


class _Net(torch.nn.Module):
    """tests/test_host_cpu.py::test_optimizer_state_survives_a_flat_layout_change's net: offsets padded to 4 floats, an order of its own."""

    def __init__(self, reorder):
        super().__init__()
        self.a = torch.nn.Linear(5, 3)
        self.b = torch.nn.Linear(3, 7)
        self.c = torch.nn.Parameter(torch.zeros(2))
        self.bn = torch.nn.BatchNorm1d(3)
        self._reorder = reorder

    def flat_param_order(self):
        ps = list(self.parameters())
        return [ps[3], ps[0], ps[6], ps[4], ps[2], ps[5], ps[1]] if self._reorder else ps


def _fill(opt):
    """By hand (no step without a device): every parameter's m, v and average carry values that name the parameter."""
    opt._ensure()
    names = [n for n, _ in _Net(False).named_parameters()]
    for name, off, n in opt.layout():
        opt.m[off:off + n] = 10.0 * (names.index(name) + 1) + torch.arange(n) * 0.01
        opt.v[off:off + n] = -opt.m[off:off + n]
        opt.ema[off:off + n] = 1000.0 + opt.m[off:off + n]
    opt.state.copy_(torch.tensor([7.0, 0.5, 0.25], dtype=torch.float64))


def _by_name(opt):
    return {name: opt.ema[off:off + n].clone() for name, off, n in opt.layout()}


def test_the_average_survives_a_flat_layout_change_by_name(capsys):
    from mmego_amd.params import FlatParams, FusedAdam
    for src_order, dst_order in ((False, True), (True, False), (True, True), (False, False)):
        src = FusedAdam(FlatParams(_Net(src_order)), ema_decay=0.75)
        dst = FusedAdam(FlatParams(_Net(dst_order)), lr=1.0, ema_decay=0.5)
        _fill(src)
        sd = src.state_dict()
        assert sd["ema_decay"] == 0.75 and torch.equal(sd["ema"], src.ema)
        dst.load_state_dict(sd)
        assert dst.ema_decay == 0.75                                        # (the saved decay wins, as lr does)
        want, got = _by_name(src), _by_name(dst)
        assert want.keys() == got.keys()
        for name in want:
            assert torch.equal(want[name], got[name]), (src_order, dst_order, name)
        # a state with an average, into an optimiser built without a decay: averaging is switched on (the max_grad_norm rule)
        off = FusedAdam(FlatParams(_Net(dst_order)))
        off.load_state_dict(sd)
        assert off.ema_decay == 0.75
        got = _by_name(off)
        for name in want:
            assert torch.equal(want[name], got[name]), (src_order, dst_order, name)
    assert "restarts" not in capsys.readouterr().out


def test_a_state_without_an_average_restarts_it_from_the_weights(capsys):
    from mmego_amd.params import FlatParams, FusedAdam
    src = FusedAdam(FlatParams(_Net(False)))
    src._ensure()
    src.m.fill_(3.0)
    dst = FusedAdam(FlatParams(_Net(True)), ema_decay=0.9)
    f = dst._ensure()
    dst.ema.fill_(-5.0)
    capsys.readouterr()
    dst.load_state_dict(src.state_dict())
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "restarts from the loaded weights" in out and "0.9" in out
    assert dst.ema_decay == 0.9 and torch.equal(dst.ema, f.flat_p) and dst.ema.data_ptr() != f.flat_p.data_ptr()


def test_averaged_exchanges_contents_and_ema_state_dict_takes_the_average():
    """Without a device (no step): the average is set by hand.  averaged() exchanges contents, never pointers, puts the weights back bit for
    bit, is not re-entrant and refuses a step; ema_state_dict() is the module's state_dict with the parameters from the average and the
    live buffers, and loads into a fresh net."""
    from mmego_amd.params import FlatParams, FusedAdam
    torch.manual_seed(3)
    net = _Net(True)
    opt = FusedAdam(FlatParams(net), ema_decay=0.5)
    f = opt._ensure()
    assert torch.equal(opt.ema, f.flat_p)                                   # (ema_0: the weights the optimiser finds)
    opt.ema.copy_(torch.randn(opt.ema.numel()))
    raw, avg = f.flat_p.clone(), opt.ema.clone()
    ptrs = (f.flat_p.data_ptr(), opt.ema.data_ptr(), net.a.weight.data_ptr())
    net.bn.running_mean.fill_(0.25)
    calls = []
    net.weights_changed = lambda: calls.append(1)
    sd = opt.ema_state_dict()
    assert list(sd.keys()) == list(net.state_dict().keys())
    with opt.averaged():
        assert len(calls) == 1 and torch.equal(f.flat_p, avg) and torch.equal(opt.ema, raw)
        assert (f.flat_p.data_ptr(), opt.ema.data_ptr(), net.a.weight.data_ptr()) == ptrs
        inside = {k: v.clone() for k, v in net.state_dict().items()}
        assert all(torch.equal(opt.ema_state_dict()[k], inside[k]) for k in inside)      # (inside the context too: the average)
        with pytest.raises(RuntimeError, match="not re-entrant"):
            with opt.averaged():
                pass
        with pytest.raises(RuntimeError, match="inside averaged"):
            opt.step()
        assert torch.equal(f.flat_p, avg)                                   # (the refused calls changed nothing)
    assert len(calls) == 2 and torch.equal(f.flat_p, raw) and torch.equal(opt.ema, avg)
    assert all(torch.equal(sd[k], inside[k]) for k in inside)
    assert torch.equal(sd["bn.running_mean"], torch.full((3,), 0.25))       # (buffers: the live ones)
    assert not torch.equal(sd["a.weight"], net.a.weight)
    fresh = _Net(False)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.b.bias, sd["b.bias"])
    with pytest.raises(ZeroDivisionError):                                  # (an exception inside the context still puts the weights back)
        with opt.averaged():
            1 / 0
    assert torch.equal(f.flat_p, raw) and torch.equal(opt.ema, avg)
    with opt.averaged():                                                    # (and the context can be entered again)
        pass
