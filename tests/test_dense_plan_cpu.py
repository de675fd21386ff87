"""CPU: the window plan of dense inference (data.DensePlan / DenseWindows) -- on the full 223-recording layout of Sample_data
(tests/golden/g11_loader.npz) the counts NOTES.md records, on hand-made recordings every property of the cover against the loop
restatement of tests/dense_ref.py -- and the command line's handling of --dense, --stride, --blend and --save_pred."""
import numpy as np
import pytest

import dense_ref as ref
import main as cli
from conftest import golden

T = 20
HAND = [5, 20, 23, 41]


@pytest.fixture(scope="module")
def snip_len():
    n = golden("g11_loader.npz")["dec.snip_len"].astype(np.int64)
    assert len(n) == 223 and n.sum() == 19114 and (n % T != 0).sum() == 214
    return n


def _reference_starts(lengths, L):
    """PosePC._read's grid, as tests/test_frame_store_cpu.py's fixtures get it from the loader: windows cut from every recording's tail."""
    starts, f0 = [], 0
    for count in lengths:
        end = f0 + int(count)
        while end - f0 >= L:
            starts.append(end - L)
            end -= L
        f0 += int(count)
    return np.asarray(starts, dtype=np.int64)


@pytest.mark.parametrize("stride,windows,max_cover", [(20, 1049, 2), (10, 1821, 3), (5, 3245, 5), (2, 7598, 11), (1, 14877, 20)])
def test_the_real_layout(snip_len, stride, windows, max_cover):
    from mmego_amd.data import DensePlan
    plan = DensePlan(snip_len, T, stride)
    assert plan.W == windows == len(plan.starts) and plan.F == 19114
    assert plan.max_cover == max_cover == plan.covered.max() and max_cover <= -(-T // stride) + 1
    assert (plan.covered == 0).sum() == 0, "every recording of the set has at least 20 frames"
    assert np.array_equal(plan.starts, ref.window_starts(snip_len, T, stride))
    rec = np.repeat(np.arange(len(snip_len)), snip_len)
    assert np.array_equal(rec[plan.starts], rec[plan.starts + T - 1]), "a window crosses a recording"
    assert np.array_equal(plan.recording, rec[plan.starts]) and np.array_equal(plan.frame_rec, rec)
    if stride == T:
        grid = _reference_starts(snip_len, T)
        assert len(grid) == 835 and np.isin(grid, plan.starts).all()
        extra = np.setdiff1d(plan.starts, grid)
        assert len(extra) == 214 and np.array_equal(extra, plan.rec_off[:-1][snip_len % T != 0])      # one head window each


def test_a_stride_beyond_the_window_is_refused(snip_len):
    from mmego_amd.data import DensePlan
    for T_, S in ((8, 10), (20, 21), (20, 0), (20, -1)):
        with pytest.raises(ValueError, match="stride"):
            DensePlan(snip_len, T_, S)
    with pytest.raises(ValueError, match="blend"):
        DensePlan(snip_len, 20, 5, "median")
    # what the refusal protects: the same rule at T = 8, S = 10 would leave 3 267 frames between windows
    starts = ref.window_starts(snip_len, 8, 10)
    seen = np.zeros(19114, dtype=bool)
    seen[(starts[:, None] + np.arange(8)).ravel()] = True
    assert (~seen).sum() == 3267


@pytest.mark.parametrize("blend", ["mean", "triangle"])
@pytest.mark.parametrize("stride", [1, 7, 20])
def test_hand_made_recordings(stride, blend):
    from mmego_amd.data import DensePlan
    plan = DensePlan(HAND, T, stride, blend)
    F = sum(HAND)
    assert plan.F == F and plan.cov_off.dtype == np.int64 and plan.cov_row.dtype == np.int32 and plan.cov_w.dtype == np.float32
    assert plan.row_frame.dtype == np.int64 and plan.row_frame.shape == (plan.W * T,)
    # the 5-frame recording: no window, no cover; every other frame is covered, at most ceil(T / S) + 1 times
    assert (plan.covered[:5] == 0).all() and (plan.starts >= 5).all()
    assert (plan.covered[5:] >= 1).all() and plan.covered.max() == plan.max_cover <= -(-T // stride) + 1
    assert np.array_equal(plan.covered, np.diff(plan.cov_off)) and plan.cov_off[0] == 0 and plan.cov_off[-1] == len(plan.cov_row)
    # starts: the rule, recording by recording, ascending; row_frame follows them
    assert np.array_equal(plan.starts, ref.window_starts(HAND, T, stride))
    assert np.array_equal(plan.row_frame.reshape(plan.W, T), plan.starts[:, None] + np.arange(T))
    bounds = np.concatenate([[0], np.cumsum(HAND)])
    for a, b in zip(bounds[:-1], bounds[1:]):
        mine = plan.starts[(plan.starts >= a) & (plan.starts < b)]
        if b - a >= T:
            assert mine[0] == a and mine[-1] == b - T and (np.diff(mine) > 0).all() and (np.diff(mine)[1:] == stride).all()
    # every (window, position) pair once; a frame's list in ascending window order, and naming rows of that frame only
    assert np.array_equal(np.sort(plan.cov_row), np.arange(plan.W * T))
    for f in range(F):
        rows = plan.cov_row[plan.cov_off[f]:plan.cov_off[f + 1]].astype(np.int64)
        assert (plan.row_frame[rows] == f).all() and (np.diff(rows // T) > 0).all()
    p = plan.cov_row % T
    assert np.array_equal(plan.cov_w, np.ones(len(p)) if blend == "mean" else np.minimum(p + 1, T - p))
    # and the whole cover against the loop restatement
    off, row, w = ref.cover(plan.starts, T, F, blend)
    assert np.array_equal(off, plan.cov_off) and np.array_equal(row, plan.cov_row) and np.array_equal(w, plan.cov_w)
    assert np.array_equal(plan.frame_in_recording, np.concatenate([np.arange(n) for n in HAND]))


def test_the_restatement_keeps_its_own_promises():
    rng = np.random.default_rng(0)
    src = rng.normal(size=(30, 45)).astype(np.float32)
    off = np.array([0, 0, 1, 4], dtype=np.int64)
    row, w = np.array([7, 3, 7, 9], dtype=np.int32), np.array([1.5, 1, 2, 1], dtype=np.float32)
    dst, spr = ref.blend(src, off, row, w)
    s64 = src.astype(np.float64)
    assert not dst[0].any() and spr[0] == 0.0                                   # no cover: zeros
    assert np.array_equal(dst[1], src[7].astype(np.float64)) and spr[1] == 0.0  # one cover: the row itself
    assert np.allclose(dst[2], (s64[3] + 2.0 * s64[7] + s64[9]) / 4.0, rtol=1e-15, atol=1e-16)
    d = np.stack([s64[3], s64[7], s64[9]]) - dst[2]
    assert np.isclose(spr[2], np.sqrt((np.array([1, 2, 1.0])[:, None] * d ** 2).sum() / (15 * 4.0)), rtol=1e-14)
    X = rng.normal(size=(40, 5))
    assert np.allclose(ref.colsum_phase(X, 8).sum(axis=0), X.sum(axis=0)) and np.array_equal(ref.colsum_phase(X, 1)[0], X.sum(axis=0))


def test_the_entry_points_are_declared_as_ops_calls_them():
    from mmego_amd import hip, ops
    protos = hip.parse_header()
    assert [n for _, n in protos["mmego_blend_windows"]] == ["stream", "src", "nrows", "C", "cov_off", "cov_row", "cov_w", "F", "dst",
                                                             "ldd", "spread"]
    assert [n for _, n in protos["mmego_colsum_phase"]] == ["stream", "X", "ldx", "rows", "C", "period", "out", "ldo"]
    assert ops.BLEND_MAX_C >= 63
    with pytest.raises(IndexError, match="outside the 4 source rows"):          # checked on the host, ahead of any launch
        ops._cover_on((np.array([0, 1], np.int64), np.array([4], np.int32), np.ones(1, np.float32)), 4, "cpu")
    with pytest.raises(ValueError, match="offsets"):
        ops._cover_on((np.array([0, 2], np.int64), np.array([1], np.int32), np.ones(1, np.float32)), 4, "cpu")


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_dense_is_a_mode_of_infer(capsys, monkeypatch):
    assert "--dense goes with --infer only" in _refused(["--dense"], capsys, monkeypatch)
    for argv in (["--dense", "--train", "--network", "Upper_Net"], ["--infer", "--dense", "--train", "--network", "Lower_Net"]):
        assert "--dense does not go with --train" in _refused(argv, capsys, monkeypatch), argv
    assert "--dense does not go with --vis" in _refused(["--infer", "--dense", "--vis"], capsys, monkeypatch)


@pytest.mark.parametrize("flag,value", [("--stride", "5"), ("--blend", "triangle"), ("--blend", "mean"), ("--save_pred", "out.npz")])
def test_dense_options_need_dense(capsys, monkeypatch, flag, value):
    for head in (["--infer"], ["--train", "--network", "Upper_Net"], []):
        assert "belongs to --infer --dense" in _refused(head + [flag, value], capsys, monkeypatch), head


@pytest.mark.parametrize("value", ["0", "-3", "21", "400"])
def test_a_stride_outside_the_window_is_refused_by_the_parser(capsys, monkeypatch, value):
    assert "[1, 20]" in _refused(["--infer", "--dense", "--stride=" + value], capsys, monkeypatch)


def test_an_unknown_blend_is_refused(capsys, monkeypatch):
    assert "invalid choice" in _refused(["--infer", "--dense", "--blend", "median"], capsys, monkeypatch)


def test_dense_options_reach_the_config():
    from mmego_amd.config import Config, ConfigDemo
    p = cli.build_parser()
    names = ("dense", "stride", "blend", "save_pred", "dense_batch_size", "upper_variant", "metrics")
    missing = object()
    keep = [(c, k, c.__dict__.get(k, missing)) for c in (ConfigDemo, Config) for k in names + ("batch_size", "resume_path", "seed")]
    assert ConfigDemo.dense is False and ConfigDemo.stride is None and ConfigDemo.blend == "mean" and ConfigDemo.save_pred is None
    try:
        for argv, want in ((["--infer", "--dense"], (True, None, "mean", None, None)),
                           (["--infer", "--dense", "--stride", "20", "--blend", "triangle", "--save_pred", "p.npz", "--batch_size", "7"],
                            (True, 20, "triangle", "p.npz", 7)),
                           (["--infer", "--dense", "--stride", "1", "--metrics", "full"], (True, 1, "mean", None, None)),
                           (["--infer"], (False, None, "mean", None, None))):
            args = p.parse_args(argv)
            cli.check_finetune(p, args, 1)
            cli.apply_overrides(args)
            assert (ConfigDemo.dense, ConfigDemo.stride, ConfigDemo.blend, ConfigDemo.save_pred, ConfigDemo.dense_batch_size) == want, argv
    finally:
        for c, k, v in keep:                         # (what the class itself held; what it inherits comes back by deleting the override)
            if v is not missing:
                setattr(c, k, v)
            elif k in c.__dict__:
                delattr(c, k)


@pytest.mark.parametrize("T", [1, 3, 20, 64])
def test_the_figure_log_has_one_named_row_per_figure(T):
    """dense.figure_rows: the names are unique, their rows disjoint, "position" spans exactly T rows and every other name one, and the
    rows fill 0 .. T + 12 -- whichever options a pass runs with."""
    from mmego_amd import dense
    assert len(set(dense.FIGURE_ROWS)) == len(dense.FIGURE_ROWS) == 13
    rows = dense.figure_rows(T)
    assert list(rows) == list(dense.FIGURE_ROWS)
    taken = {name: list(range(r.start, r.stop)) if isinstance(r, slice) else [r] for name, r in rows.items()}
    assert len(taken["position"]) == T and all(len(v) == 1 for name, v in taken.items() if name != "position")
    every = sorted(r for v in taken.values() for r in v)
    assert every == list(range(T + 12))                 # disjoint, no gap, T + 12 in all
