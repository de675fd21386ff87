"""CPU: data.FrameStore's host side on the full 19 114-frame layout of Sample_data (tests/golden/g11_loader.npz, built as
tests/test_data_cpu.py builds it) -- who owns a frame, which window starts are valid, the jittered draws -- the numpy restatement of
mmego_pack_frames (tests/frame_pack_ref.py) held to its own properties, and the command line's handling of --window_jitter and
--point_keep."""
import numpy as np
import pytest

import frame_pack_ref as ref
import main as cli
from conftest import golden
from test_data_cpu import _decoded

L = 20


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    """(the training PosePC of the whole layout with its per-frame views, its FrameStore with jitter on; host tensors)."""
    from mmego_amd.config import Config
    from mmego_amd.data import FrameStore, PosePC
    dec = _decoded(golden("g11_loader.npz"), golden("real16.npz"))
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(PosePC, "_decode", lambda self: dec)
        mp.setattr(Config, "data_root", str(tmp_path_factory.mktemp("Sample_data")))
        assert Config.dataset_random_seed == 1
        np.random.seed(0)
        ds = PosePC(train=True, batch_length=L, keep_frames=True)
        np.random.seed(0)
        plain = PosePC(train=True, batch_length=L)
    finally:
        mp.undo()
    return ds, plain, FrameStore(ds, "cpu", jitter=True, seed=5)


def test_keeping_the_frames_changes_nothing_else(loaded):
    ds, plain, _ = loaded
    assert plain.frame_packed_ is None and ds.frame_packed_.shape == (19114, 128, 6) and ds.frame_packed_.dtype == np.float32
    for name in ("data_ti_", "data_key_", "imu_", "skl_", "R_R0R_", "win_start_"):
        assert np.array_equal(getattr(ds, name), getattr(plain, name)), name
    assert len(ds) == len(plain) == 668 and len(ds.win_start_) == 835 and ds.split_cut == 668
    assert len(ds.frame_rec_) == 19114 and ds.frame_rec_[-1] == 222 and ds.frame_pts_.shape[1] == 5


def test_owner_map_and_valid_starts(loaded):
    ds, _, fs = loaded
    rec, own = ds.frame_rec_, fs.owner
    assert (own == fs.TRAIN).sum() == 668 * L and (own == fs.TEST).sum() == 167 * L and (own == fs.UNUSED).sum() == 2414
    valid = fs.valid_starts()
    assert len(valid) == 9992
    span = valid[:, None] + np.arange(L)
    assert (rec[span] == rec[valid][:, None]).all(), "a valid start crosses a recording"
    assert not (own[span] == fs.TEST).any(), "a valid start touches a test frame"
    # and no start outside the list qualifies
    others = np.setdiff1d(np.arange(len(rec) - L + 1), valid)
    span = others[:, None] + np.arange(L)
    assert ((rec[span] != rec[others][:, None]).any(axis=1) | (own[span] == fs.TEST).any(axis=1)).all()
    assert np.isin(fs.ref_starts, valid).all(), "every reference training window is itself a valid start"
    assert fs.n == 668 and fs.n - fs.n_movable == 55
    assert abs(float(np.mean(fs._cand_len)) - 26.0) < 0.5          # (mean freedom per window: about 26 starts)


def test_jitter_off_is_the_reference(loaded):
    from mmego_amd.data import FrameStore
    ds, _, _ = loaded
    fs = FrameStore(ds, "cpu")
    for epoch in (0, 3):
        starts = fs.begin_epoch(epoch)
        assert np.array_equal(starts, ds.win_start_[:668])
    idx = starts[:, None] + np.arange(L)
    assert np.array_equal(ds.frame_packed_[idx], ds.data_ti_[:668])
    assert np.array_equal(ds.frame_imu_[idx], ds.imu_[:668])
    assert np.array_equal(ds.frame_key_[idx], ds.data_key_[:668])
    assert np.array_equal(ds.frame_R_[idx], ds.R_R0R_[:668])
    assert np.array_equal(np.broadcast_to(ds.frame_bones_, ds.skl_[:668].shape), ds.skl_[:668])
    assert np.array_equal(fs.frame_index([3, 1]), np.concatenate([starts[3] + np.arange(L), starts[1] + np.arange(L)]))
    # the test windows too, for the owner map
    tidx = ds.win_start_[668:, None] + np.arange(L)
    assert np.array_equal(ds.frame_packed_[tidx], ds.data_ti_[668:])


def test_jitter_on(loaded):
    from mmego_amd.data import FrameStore, batch_indices
    ds, _, fs = loaded
    valid = set(fs.valid_starts().tolist())
    state = np.random.get_state()
    draws = {}
    for epoch in (0, 1, 2):
        s = fs.begin_epoch(epoch).copy()
        assert set(s.tolist()) <= valid and (np.abs(s - fs.ref_starts) <= L - 1).all()
        assert np.array_equal(s[fs._cand_len == 1], fs.ref_starts[fs._cand_len == 1])
        draws[epoch] = s
    assert np.array_equal(state[1], np.random.get_state()[1]), "the draws leave numpy's global generator alone"
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    assert (draws[0] != fs.ref_starts).sum() > 500                   # (most of the 613 movable windows move)
    again = FrameStore(ds, "cpu", jitter=True, seed=5)
    assert np.array_equal(again.begin_epoch(1), draws[1]) and np.array_equal(again.begin_epoch(0), draws[0])     # a function of (seed, epoch)
    assert not np.array_equal(FrameStore(ds, "cpu", jitter=True, seed=6).begin_epoch(1), draws[1])
    # the minibatch order of the trainers' generator is the same with the option on and off
    rng_on, rng_off = np.random.RandomState(1234), np.random.RandomState(1234)
    for epoch in (0, 1):
        fs.begin_epoch(epoch)
        on = [i.copy() for i in batch_indices(fs.n, 64, True, rng_on)]
        fs.frame_index(on[0])
        off = [i.copy() for i in batch_indices(668, 64, True, rng_off)]
        assert len(on) == len(off) and all(np.array_equal(a, b) for a, b in zip(on, off))


@pytest.mark.parametrize("keep_p", [1.0, 0.5, 0.01])
def test_the_restatement_keeps_its_own_promises(keep_p):
    rng = np.random.default_rng(0)
    pc_no = 128
    for n in (1, 3, 127, 128, 129, 174):
        raw = rng.normal(size=(n, 5)).astype(np.float32)
        conv = ref.convert(raw)
        for q in range(6):
            out, who = ref.pack_frame(raw, q, pc_no, 174, keep_p, seed=11)
            kept = ref.kept_points(n, q, keep_p, 11)
            assert len(kept) >= 1 and (np.diff(kept) > 0).all() and kept.max() < n, "a frame is never emptied"
            if keep_p == 1.0:
                assert np.array_equal(kept, np.arange(n))
            placed = who[who >= 0]
            assert len(set(placed.tolist())) == len(placed), "no point twice"
            if len(kept) < pc_no:
                assert sorted(placed.tolist()) == kept.tolist()              # exactly the survivors, each once
                assert np.array_equal(out[who < 0], np.zeros(((who < 0).sum(), 6), np.float32))
            else:
                assert len(placed) == pc_no and set(placed.tolist()) <= set(kept.tolist())
            assert np.array_equal(out[who >= 0], conv[placed])
    # the keep stream and the ordering stream are distinct, and q is a counter: other frames, other draws
    a, b = ref.pack_frame(raw, 0, pc_no, 174, 1.0, 11)[1], ref.pack_frame(raw, 1, pc_no, 174, 1.0, 11)[1]
    assert not np.array_equal(a, b)
    assert ref.dropout_key(11, ref.SALT_KEEP) != ref.dropout_key(11, ref.SALT_ORDER)


def test_pack_frames_is_declared_as_ops_calls_it():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_pack_frames"]] == ["stream", "pts", "frame_off", "frame_idx", "nout", "pc_no", "max_n", "keep_p",
                                                           "seed", "out"]
    import ctypes
    assert protos["mmego_pack_frames"][8][0] is ctypes.c_ulonglong and protos["mmego_pack_frames"][7][0] is ctypes.c_float
    assert ops.pack_frames_max_n(128) == 2048 and ops.pack_frames_max_n(1024) == 2048 and ops.PACK_FRAMES_MAX_PC_NO == 1024


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_options_are_refused_outside_training(capsys, monkeypatch):
    for argv in (["--infer", "--window_jitter"], ["--infer", "--point_keep", "0.8"], ["--window_jitter"], ["--point_keep", "0.8"],
                 ["--train", "--infer", "--network", "Upper_Net", "--window_jitter"]):
        assert "go with --train only" in _refused(argv, capsys, monkeypatch), argv


def test_point_keep_is_refused_for_stage_1(capsys, monkeypatch):
    err = _refused(["--train", "--network", "IMU_Net", "--point_keep", "0.8"], capsys, monkeypatch)
    assert "--point_keep does not go with --network IMU_Net" in err


@pytest.mark.parametrize("value", ["0", "-0.5", "1.5", "nan", "inf"])
def test_point_keep_outside_the_unit_interval_is_refused(capsys, monkeypatch, value):
    for net in ("Upper_Net", "Lower_Net"):
        assert "(0, 1]" in _refused(["--train", "--network", net, "--point_keep=" + value], capsys, monkeypatch)


def test_options_reach_the_config():
    from mmego_amd.config import Config
    p = cli.build_parser()
    names = ("window_jitter", "point_keep", "seed", "finetune_imu", "finetune_upper", "finetune_all", "imu_lr", "upper_lr", "imu_dropout",
             "resume_path", "upper_variant", "clip_grad_norm")
    keep = {k: getattr(Config, k, None) for k in names}
    assert Config.window_jitter is False and Config.point_keep is None          # (the defaults: DeviceArrays, as before)
    try:
        for argv, jitter, pk in ((["--train", "--network", "IMU_Net", "--window_jitter"], True, None),
                                 (["--train", "--network", "Upper_Net", "--window_jitter", "--point_keep", "0.8", "--seed", "3"], True, 0.8),
                                 (["--train", "--network", "Upper_Net", "--upper_variant", "wlocal", "--point_keep", "1"], False, 1.0),
                                 (["--train", "--network", "Upper_Net", "--finetune_imu", "--point_keep", "0.5"], False, 0.5),
                                 (["--train", "--network", "Lower_Net", "--finetune_upper", "--window_jitter"], True, None),
                                 (["--train", "--network", "Lower_Net", "--finetune_all", "--point_keep", "0.9"], False, 0.9),
                                 (["--train", "--network", "Lower_Net"], False, None)):
            args = p.parse_args(argv)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert Config.window_jitter is jitter and Config.point_keep == pk, argv
            assert Config.seed == (3 if "--seed" in argv else None)
    finally:
        for k, v in keep.items():
            setattr(Config, k, v)
