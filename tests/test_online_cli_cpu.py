"""CPU: --online / --lookahead and --one_euro / --one_euro_beta / --one_euro_dcutoff on the command line (defaults, the stride default
under --online, refusals with their messages, what reaches ConfigDemo), the checks of dense_infer's online and one_euro arguments, and
the two entry points' declarations."""
import numpy as np
import pytest

import main as cli


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_the_flags_reach_the_config_and_are_off_by_default():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "upper_variant", "metrics", "smooth", "rot_smooth",
             "online", "one_euro", "floor", "breakdown", "vis", "render")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    assert ConfigDemo.online is None and ConfigDemo.one_euro is None
    half = Config.frame_no // 2
    try:
        for argv, online, stride, euro in (
                (["--infer", "--dense", "--online"], 0, 1, None),
                (["--infer", "--dense", "--online", "--lookahead", "4"], 4, min(5, half), None),
                (["--infer", "--dense", "--online", "--lookahead", str(Config.frame_no - 1)], Config.frame_no - 1, half, None),
                (["--infer", "--dense", "--online", "--lookahead", "4", "--stride", "2"], 4, 2, None),
                (["--infer", "--dense", "--one_euro", "0.05"], None, None, (0.05, 0.0, 0.1)),
                (["--infer", "--dense", "--stride", "7", "--one_euro", "0.5", "--one_euro_beta", "10", "--one_euro_dcutoff", "0.2"],
                 None, 7, (0.5, 10.0, 0.2)),
                (["--infer", "--dense", "--online", "--blend_space", "bones", "--one_euro", "1"], 0, 1, (1.0, 0.0, 0.1)),
                (["--infer", "--dense"], None, None, None), (["--infer"], None, None, None)):
            args = p.parse_args(argv)
            cli.check_dense(p, args)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert (ConfigDemo.online, ConfigDemo.stride, ConfigDemo.one_euro) == (online, stride, euro), argv
    finally:
        for c, k, v in keep:                         # (what the class itself held; what it inherits comes back by deleting the override)
            if v is not missing:
                setattr(c, k, v)
            elif k in c.__dict__:
                delattr(c, k)
    args = p.parse_args(["--infer", "--dense"])
    assert args.online is False and args.lookahead is None
    assert args.one_euro is None and args.one_euro_beta is None and args.one_euro_dcutoff is None


@pytest.mark.parametrize("flag", [["--online"], ["--lookahead", "2"], ["--one_euro", "0.1"], ["--one_euro_beta", "1"],
                                  ["--one_euro_dcutoff", "0.2"]])
def test_the_flags_need_infer_dense(capsys, monkeypatch, flag):
    for head in (["--infer"], ["--train", "--network", "Upper_Net"], []):
        err = _refused(head + flag, capsys, monkeypatch)
        assert "%s belongs to --infer --dense" % flag[0] in err, head


def test_what_belongs_to_what(capsys, monkeypatch):
    assert "--lookahead belongs to --online" in _refused(["--infer", "--dense", "--lookahead", "2"], capsys, monkeypatch)
    for flag in (["--one_euro_beta", "1"], ["--one_euro_dcutoff", "0.2"]):
        assert "%s belongs to --one_euro FC" % flag[0] in _refused(["--infer", "--dense"] + flag, capsys, monkeypatch)


def test_values_out_of_range_are_refused(capsys, monkeypatch):
    from mmego_amd.config import Config
    head = ["--infer", "--dense"]
    for L in ("-1", str(Config.frame_no)):
        assert "--lookahead is the latency budget in frames" in _refused(head + ["--online", "--lookahead=" + L], capsys, monkeypatch)
    assert "invalid int value" in _refused(head + ["--online", "--lookahead", "1.5"], capsys, monkeypatch)
    for v in ("0", "-0.1", "nan", "inf"):
        assert "--one_euro is the filter's minimum cutoff" in _refused(head + ["--one_euro=" + v], capsys, monkeypatch)
        assert "--one_euro_dcutoff is the speed estimate's cutoff" in _refused(head + ["--one_euro", "1", "--one_euro_dcutoff=" + v],
                                                                             capsys, monkeypatch)
    for v in ("-0.1", "nan", "inf"):
        assert "--one_euro_beta is the speed coefficient" in _refused(head + ["--one_euro", "1", "--one_euro_beta=" + v], capsys, monkeypatch)
    assert "invalid float value" in _refused(head + ["--one_euro", "fast"], capsys, monkeypatch)


def test_the_stride_under_online(capsys, monkeypatch):
    err = _refused(["--infer", "--dense", "--online", "--stride", "2"], capsys, monkeypatch)
    assert "--stride has to lie in [1, 1] under --online --lookahead 0" in err and "uncovered" in err
    err = _refused(["--infer", "--dense", "--online", "--lookahead", "3", "--stride", "5"], capsys, monkeypatch)
    assert "--stride has to lie in [1, 4] under --online --lookahead 3" in err


def test_combinations_that_are_refused(capsys, monkeypatch):
    head = ["--infer", "--dense"]
    assert "--online does not go with --smooth" in _refused(head + ["--online", "--smooth", "4"], capsys, monkeypatch)
    assert "--online does not go with --rot_smooth" in _refused(head + ["--online", "--blend_space", "rot", "--rot_smooth", "4"],
                                                                capsys, monkeypatch)
    assert "--one_euro does not go with --smooth" in _refused(head + ["--one_euro", "1", "--smooth", "4"], capsys, monkeypatch)
    assert "--one_euro does not go with --rot_smooth" in _refused(head + ["--one_euro", "1", "--blend_space", "rot", "--rot_smooth", "4"],
                                                                  capsys, monkeypatch)
    assert "--one_euro does not go with --blend_space rot" in _refused(head + ["--one_euro", "1", "--blend_space", "rot"], capsys, monkeypatch)


def test_the_arguments_of_dense_infer_are_checked():
    from mmego_amd import dense
    assert dense._check_online(None, 20) is None and dense._check_online(np.int64(3), 20) == 3 and dense._check_online(19, 20) == 19
    for bad in (-1, 20, 2.0, True, "0"):
        with pytest.raises(ValueError, match="online"):
            dense._check_online(bad, 20)
    assert dense._check_one_euro(None) is None and dense._check_one_euro((1, np.float32(0.0), 0.5)) == (1.0, 0.0, 0.5)
    for bad in ((1.0, 0.0), (0.0, 0.0, 0.1), (-1.0, 0.0, 0.1), (1.0, -0.5, 0.1), (1.0, 0.0, 0.0), (float("nan"), 0.0, 0.1),
                (1.0, float("inf"), 0.1), (1.0, 0.0, float("nan")), (True, 0.0, 0.1), ("1", 0.0, 0.1), 0.05):
        with pytest.raises(ValueError, match="one_euro"):
            dense._check_one_euro(bad)

    class _DS:
        frame_no = 20
    # refused ahead of any device work: nothing below reaches the plan
    for kw, match in ((dict(online=0, smooth=(4, 2, "gauss")), "online: smooth reads H frames ahead"),
                      (dict(online=0, blend_space="rot", rot_smooth=(4, 2, "gauss")), "online: rot_smooth reads H frames ahead"),
                      (dict(one_euro=(1.0, 0.0, 0.1), smooth=(4, 2, "gauss")), "one_euro: it sits where smooth sits"),
                      (dict(one_euro=(1.0, 0.0, 0.1), blend_space="rot", rot_smooth=(4, 2, "gauss")), "one_euro: it sits where rot_smooth"),
                      (dict(one_euro=(1.0, 0.0, 0.1), blend_space="rot"), "one_euro: the filter runs on joint positions"),
                      (dict(online=20), "online: the lookahead"), (dict(online=2, stride=4), "online: frame f is served"),
                      (dict(one_euro=(0.0, 0.0, 0.1)), "one_euro: fc")):
        stride = kw.pop("stride", 1)
        with pytest.raises(ValueError, match=match):
            dense.dense_infer(None, None, None, None, _DS(), stride, **kw)


def test_the_entry_points_are_declared_as_ops_calls_them():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_one_euro"]] == ["stream", "src", "lds", "F", "J", "run_off", "run_on", "R", "fc", "beta", "dc", "dst",
                                                        "ldd", "moved"]
    assert [n for _, n in protos["mmego_one_euro_bones"]] == ["stream", "src", "lds", "F", "J", "run_off", "run_on", "R", "fc", "beta", "dc",
                                                              "bones", "bone_len", "NB", "dst", "ldd", "moved", "fallback"]
    import ctypes
    assert [t for t, n in protos["mmego_one_euro"] if n in ("fc", "beta", "dc")] == [ctypes.c_double] * 3
    assert callable(ops.one_euro) and callable(ops.one_euro_bones) and callable(ops.one_euro_runs)
