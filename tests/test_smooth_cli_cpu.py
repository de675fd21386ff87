"""CPU: --smooth / --smooth_order / --smooth_taper on the command line (defaults, refusals, what reaches ConfigDemo), the weight tables
of dense.smooth_weights, the check of dense_infer's smooth argument, and the two entry points' declarations."""
import numpy as np
import pytest

import main as cli
import smooth_ref as sref


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_smooth_reaches_the_config_and_is_off_by_default():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "blend_space", "save_pred", "dense_batch_size", "upper_variant", "metrics", "smooth")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    assert ConfigDemo.smooth is None
    try:
        for argv, want in ((["--infer", "--dense", "--smooth", "4"], (4, 2, "gauss")),
                           (["--infer", "--dense", "--smooth", "1", "--smooth_order", "0"], (1, 0, "gauss")),
                           (["--infer", "--dense", "--smooth", "31", "--smooth_taper", "box", "--smooth_order", "1"], (31, 1, "box")),
                           (["--infer", "--dense", "--blend_space", "bones", "--smooth", "8", "--smooth_taper", "gauss"], (8, 2, "gauss")),
                           (["--infer", "--dense"], None), (["--infer"], None)):
            args = p.parse_args(argv)
            cli.check_dense(p, args)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert ConfigDemo.smooth == want, argv
    finally:
        for c, k, v in keep:                         # (what the class itself held; what it inherits comes back by deleting the override)
            if v is not missing:
                setattr(c, k, v)
            elif k in c.__dict__:
                delattr(c, k)
    args = p.parse_args(["--infer", "--dense"])
    assert args.smooth is None and args.smooth_order is None and args.smooth_taper is None


@pytest.mark.parametrize("flag", [["--smooth", "4"], ["--smooth_order", "1"], ["--smooth_taper", "box"]])
def test_the_smooth_flags_need_dense(capsys, monkeypatch, flag):
    for head in (["--infer"], ["--train", "--network", "Upper_Net"], []):
        err = _refused(head + flag, capsys, monkeypatch)
        assert "%s belongs to --infer --dense" % flag[0] in err, head


@pytest.mark.parametrize("flag", [["--smooth_order", "1"], ["--smooth_taper", "box"]])
def test_order_and_taper_need_smooth(capsys, monkeypatch, flag):
    assert "%s belongs to --smooth H" % flag[0] in _refused(["--infer", "--dense"] + flag, capsys, monkeypatch)


@pytest.mark.parametrize("H", ["0", "32", "-3"])
def test_a_half_width_outside_1_to_31_is_refused(capsys, monkeypatch, H):
    assert "--smooth is the filter's half-width in frames" in _refused(["--infer", "--dense", "--smooth", H], capsys, monkeypatch)


def test_other_values_are_refused(capsys, monkeypatch):
    assert "invalid choice" in _refused(["--infer", "--dense", "--smooth", "4", "--smooth_order", "3"], capsys, monkeypatch)
    assert "invalid choice" in _refused(["--infer", "--dense", "--smooth", "4", "--smooth_taper", "hann"], capsys, monkeypatch)
    assert "invalid int value" in _refused(["--infer", "--dense", "--smooth", "2.5"], capsys, monkeypatch)


def test_weight_tables():
    from mmego_amd import dense
    for H in (1, 2, 8, 31):
        box, gauss = dense.smooth_weights(H, "box"), dense.smooth_weights(H, "gauss")
        assert box.dtype == np.float32 and gauss.dtype == np.float32 and box.shape == gauss.shape == (2 * H + 1,)
        assert np.array_equal(box, np.ones(2 * H + 1, np.float32))
        k = np.arange(-H, H + 1, dtype=np.float64)
        assert np.array_equal(gauss, np.exp(-2.0 * k * k / (H * H)).astype(np.float32))
        assert gauss[H] == 1.0 and np.array_equal(gauss, gauss[::-1]) and (gauss > 0.13).all()
        assert np.array_equal(box, sref.weights(H, "box")) and np.array_equal(gauss, sref.weights(H, "gauss"))
    for H, taper in ((0, "box"), (32, "box"), (2.0, "box"), (True, "box"), (4, "hann")):
        with pytest.raises(ValueError, match="smooth"):
            dense.smooth_weights(H, taper)


def test_the_smooth_argument_is_checked():
    from mmego_amd import dense
    assert dense._check_smooth(None) is None
    assert dense._check_smooth((np.int64(3), 2, "box")) == (3, 2, "box")
    for bad in ((3, 2), (0, 2, "box"), (32, 2, "box"), (3, 3, "box"), (3, -1, "box"), (3, 1.0, "box"), (3, 2, "hann"), "gauss", 3):
        with pytest.raises(ValueError, match="smooth"):
            dense._check_smooth(bad)


def test_the_entry_points_are_declared_as_ops_calls_them():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_smooth_frames"]] == ["stream", "src", "lds", "F", "C", "seg", "w", "H", "D", "dst", "ldd", "moved"]
    assert [n for _, n in protos["mmego_smooth_bones"]] == ["stream", "src", "lds", "F", "J", "seg", "w", "H", "D", "bones", "bone_len",
                                                            "NB", "dst", "ldd", "moved", "fallback"]
    assert callable(ops.smooth_frames) and callable(ops.smooth_bones) and ops.SMOOTH_MAX_H == 31
