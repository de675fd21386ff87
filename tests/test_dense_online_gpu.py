"""GPU: dense inference's causal options (dense.dense_infer with online=L and one_euro=(fc, beta, dc); `main.py --infer --dense --online
--one_euro`) on the synthetic tree of tests/test_dense_infer_gpu.py: recordings of 23, 20, 7 and 41 frames, frame_no = 20.

What is compared with what: a pass with both keywords None, and one with online = frame_no - 1, with the pass without them (bytes); at
online = 0 and stride 1 every covered frame with the one window row that ends at it (bytes); at online = 2 and stride 3 the blended
frames with a numpy blend over a cover built here from the definition (2e-5 m, the project's joint parity bound); the filtered frames
with tests/one_euro_ref.py applied to the downloaded blended frames recording by recording (2e-5 m); filtered bones with the body's
lengths (2e-6 m, the bar of tests/test_smooth_bones_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import dense_ref as ref
import one_euro_ref as oref
from conftest import ROOT
from test_dense_infer_gpu import LENGTHS, F, T, _run, world       # noqa: F401  (world: the module-scoped fixture, built once here)

pytestmark = pytest.mark.gpu

EURO = (0.05, 10.0, 0.1)
REC_OFF = np.concatenate([[0], np.cumsum(LENGTHS)])
LONG = [r for r, n in enumerate(LENGTHS) if n >= T]


def run(world, stride, **kw):
    from mmego_amd import dense
    key = ("online", stride) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in world.runs:
        s, a = dense.dense_infer(world.base, None, world.up, world.lo, world.ds, stride, batch_size=4, **kw)
        world.runs[key] = (s, dict(a, win_up_h=a["win_up"].cpu().numpy(), win_lo_h=a["win_lo"].cpu().numpy()))
    return world.runs[key]


def same(x, y):
    if isinstance(x, torch.Tensor):
        return isinstance(y, torch.Tensor) and torch.equal(x, y)
    if isinstance(x, np.ndarray):
        return isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(same(a, b) for a, b in zip(x, y))
    return x == y or (x != x and y != y)


def same_dicts(a, b, skip=("plan",)):
    assert set(a) == set(b)
    for k in a:
        assert k in skip or same(a[k], b[k]), k


def test_none_is_the_pass_without_the_keywords(world):
    s0, a0 = world.run(3, "mean", 4)
    s1, a1 = run(world, 3, online=None, one_euro=None)
    same_dicts(s0, s1)
    same_dicts({k: v for k, v in a0.items()}, a1)


@pytest.mark.parametrize("metrics", ["reference", "full"])
def test_the_full_lookahead_is_the_offline_pass(world, metrics):
    s0, a0 = world.run(3, "mean", 4, metrics)
    s1, a1 = run(world, 3, online=T - 1, metrics=metrics)
    assert set(s1) - set(s0) == {"online", "warmup_frames"} and s1["online"] == T - 1 and s1["warmup_frames"] == 0
    same_dicts(s0, {k: v for k, v in s1.items() if k not in ("online", "warmup_frames")})
    same_dicts(a0, a1)


def test_lookahead_0_at_stride_1_is_the_row_that_ends_at_the_frame(world):
    s, a = run(world, 1, online=0)
    plan = a["plan"]
    assert plan.W == 4 + 1 + 22 and s["online"] == 0 and s["warmup_frames"] == 57 and s["max_cover"] == 1 and s["stride"] == 1
    warm = np.zeros(F, bool)
    for r in LONG:
        warm[REC_OFF[r]:REC_OFF[r] + T - 1] = True
    short = a["recording"] == 2
    assert warm.sum() == 57 and np.array_equal(a["covered"] == 0, warm | short) and s["covered_frames"] == F - 57 - 7
    assert np.isnan(a["pred"][warm | short]).all() and not np.isnan(a["pred"][~(warm | short)]).any()
    cov = np.flatnonzero(a["covered"])
    ends = (np.arange(plan.W) * T + T - 1)                                     # every window's last row
    rows = ends[np.searchsorted(plan.row_frame[ends], cov)]
    assert np.array_equal(plan.row_frame[rows], cov) and np.array_equal(plan.cov_row, rows)
    assert a["upper"][cov].tobytes() == a["win_up_h"][rows].tobytes() and a["lower"][cov].tobytes() == a["win_lo_h"][rows].tobytes()
    assert (a["spread"] == 0.0).all()
    # the figures are means over the covered frames alone
    allj = np.linalg.norm(a["pred"][cov].astype(np.float64) - a["target"][cov], axis=2).mean() * 100
    assert abs(s["all_cm"] - allj) <= 1e-3


@pytest.mark.parametrize("blend", ["mean", "triangle"])
def test_lookahead_2_at_stride_3_against_a_numpy_blend(world, blend):
    L = 2
    s, a = run(world, 3, online=L, blend=blend)
    plan = a["plan"]
    off, rows, wts = [0], [], []                                               # the cover from the definition
    for f in range(F):
        for w in np.flatnonzero((plan.starts <= f) & (f < plan.starts + T) & (plan.starts + T - 1 <= f + L)):
            p = f - plan.starts[w]
            rows.append(w * T + p)
            wts.append(1.0 if blend == "mean" else float(min(p + 1, T - p)))
        off.append(len(rows))
    off, rows, wts = np.asarray(off), np.asarray(rows), np.asarray(wts)
    cov = np.diff(off) > 0
    assert np.array_equal(a["covered"], np.diff(off)) and s["warmup_frames"] == 3 * (T - 1 - L) and cov.sum() == F - 7 - 51
    up64, spr64 = ref.blend(a["win_up_h"], off, rows, wts)
    lo64, _ = ref.blend(a["win_lo_h"], off, rows, wts, spread=False)
    diff = np.abs(a["pred"][cov] - ref.assemble(up64, lo64)[cov]).max()
    print("online 2, stride 3, %s: pred differs from the numpy blend by at most %.3e m" % (blend, diff))
    assert diff <= 2e-5 and np.isnan(a["pred"][~cov]).all()
    assert abs(s["spread_cm"] - spr64[cov].mean() * 100) <= 1e-3


def _filtered(blended, covered):
    """one_euro_ref over every recording's covered stretch of the blended rows [F, J, 3]."""
    want = blended.astype(np.float64)
    for r in range(len(LENGTHS)):
        m = np.flatnonzero(covered[REC_OFF[r]:REC_OFF[r + 1]] != 0) + REC_OFF[r]
        if len(m):
            assert np.array_equal(m, np.arange(m[0], m[-1] + 1))               # (one stretch per recording here)
            want[m] = oref.filter_vectors(blended[m], *EURO)
    return want


@pytest.mark.parametrize("metrics", ["reference", "full"])
def test_one_euro_against_the_restatement(world, metrics):
    s0, a0 = world.run(3, "mean", 4, metrics)
    s, a = run(world, 3, one_euro=EURO, metrics=metrics)
    cov = a["covered"] > 0
    for name in ("upper", "lower"):
        diff = np.abs(a[name][cov] - _filtered(a0[name], a0["covered"])[cov]).max()
        print("one_euro %s: differs from the restatement by at most %.3e m" % (name, diff))
        assert diff <= 2e-5
        assert (a[name][cov] != a0[name][cov]).mean() > 0.9, "the filter ran"
    # the blended frames keep their figures and their bytes
    assert a["pred_unsmoothed"].tobytes() == a0["pred"].tobytes()
    for k in ("all_cm", "upper_cm", "lower_cm", "rot_deg", "per_joint_cm") + (("accel_cm",) if metrics == "full" else ()):
        assert same(s["unsmoothed_" + k], s0[k]), k
    for k in ("single_all_cm", "spread_cm", "position_cm", "windows", "covered_frames"):
        assert same(s[k], s0[k]), k
    assert s["one_euro"] == EURO and s["one_euro_fallback"] == 0 and "smooth" not in s and set(a) - set(a0) == {"pred_unsmoothed", "moved"}
    want_m = np.sqrt(((a["upper"].astype(np.float64) - a0["upper"]) ** 2).sum(axis=(1, 2)) / 15)
    assert np.abs(a["moved"] - want_m).max() <= 2e-5 and abs(s["moved_cm"] - want_m[cov].mean() * 100) <= 1e-3
    allj = np.linalg.norm(a["pred"][cov].astype(np.float64) - a["target"][cov], axis=2).mean() * 100
    assert abs(s["all_cm"] - allj) <= 1e-3 and s["all_cm"] != s0["all_cm"]


def test_one_euro_under_bones_keeps_the_bone_lengths(world):
    from mmego_amd import dense, skeleton
    s, a = run(world, 3, one_euro=EURO, blend_space="bones")
    cov = a["covered"] > 0
    Lu, Ll = dense.bone_lengths(a["plan"].bone_set)
    worst = 0.0
    for rows, walk, L in ((a["upper"], np.asarray(skeleton.WALK_UPPER), Lu), (a["lower"], np.asarray(skeleton.WALK_LOWER), Ll)):
        x = rows[cov].astype(np.float64)
        worst = max(worst, np.abs(np.linalg.norm(x[:, walk[:, 0]] - x[:, walk[:, 1]], axis=2) - L.astype(np.float64)).max())
    print("one_euro under bones: worst | |bone| - L | %.3e m" % worst)
    assert worst <= 2e-6 and s["one_euro"] == EURO and s["one_euro_fallback"] == 0 and s["blend_space"] == "bones"
    _, a0 = run(world, 3, blend_space="bones")
    assert a["pred_unsmoothed"].tobytes() == a0["pred"].tobytes() and (a["pred"][cov] != a0["pred"][cov]).mean() > 0.5


def test_one_euro_starts_behind_the_warm_up(world):
    s0, a0 = run(world, 1, online=0)
    s, a = run(world, 1, online=0, one_euro=EURO)
    assert np.array_equal(a["covered"], a0["covered"]) and s["warmup_frames"] == 57 and s["online"] == 0
    firsts = np.asarray([REC_OFF[r] + T - 1 for r in LONG])
    assert (a["covered"][firsts] == 1).all() and (a["covered"][firsts - 1] == 0).all()
    assert a["pred"][firsts].tobytes() == a0["pred"][firsts].tobytes() and (a["moved"][firsts] == 0.0).all()
    assert np.isnan(a["pred"][a["covered"] == 0]).all() and (a["moved"][a["covered"] == 0] == 0.0).all()
    cov = a["covered"] > 0
    for name in ("upper", "lower"):
        assert np.abs(a[name][cov] - _filtered(a0[name], a0["covered"])[cov]).max() <= 2e-5


def test_refused_combinations(world):
    from mmego_amd import dense
    for kw, match in ((dict(online=0, smooth=(4, 2, "gauss")), "online: smooth"),
                      (dict(online=0, blend_space="rot", rot_smooth=(4, 2, "gauss")), "online: rot_smooth"),
                      (dict(one_euro=EURO, smooth=(4, 2, "gauss")), "one_euro"), (dict(one_euro=EURO, blend_space="rot"), "one_euro"),
                      (dict(one_euro=EURO, blend_space="rot", rot_smooth=(4, 2, "gauss")), "one_euro"),
                      (dict(online=1, stride=3), "online: frame f is served"), (dict(online=T), "online"), (dict(online=-1), "online"),
                      (dict(one_euro=(0.0, 0.0, 0.1)), "one_euro"), (dict(one_euro=(1.0, float("nan"), 0.1)), "one_euro")):
        stride = kw.pop("stride", 1)
        with pytest.raises(ValueError, match=match):
            dense.dense_infer(world.base, None, world.up, world.lo, world.ds, stride, batch_size=4, **kw)


def test_command_line_prints_the_lines_and_writes_the_keys(world):
    """One `main.py --infer --dense --online --lookahead 2 --one_euro 0.05 --one_euro_beta 10 --metrics full --save_pred` run in a
    fresh child process: the stride defaults to 3."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    path = str(world.tmp / "online.npz")
    out = _run(["--infer", "--dense", "--online", "--lookahead", "2", "--one_euro", "0.05", "--one_euro_beta", "10", "--metrics", "full",
                "--save_pred", path, "--gt_head_pose", "--data_root", world.data, "--device", "cuda:0", "--seed", "3", "--batch_size", "4",
                "--load_Upper_path", str(world.tmp / "upper.pth"), "--load_Lower_path", str(world.tmp / "lower.pth")], env)
    lines = ["Average Joint Localization Error(cm):", "Window Disagreement(cm):",
             "Online: lookahead 2 frames (frame f from the windows that ended by f + 2), warm-up frames 51",
             "Dense windows: 11 windows of 20 frames at stride 3 (blend mean), 33 of 91 frames covered, largest cover 1, lookahead 2, "
             "warm-up frames 51", "Per-frame skeletons saved in", "Unsmoothed (blended) Error(cm): all ",
             "One-Euro Filter: displacement(cm) ", "Unsmoothed Acceleration Error(cm/frame^2): "]
    at = [out.index(line) for line in lines]
    assert at == sorted(at), "the lines come in this order"
    assert "(min cutoff 0.05 beta 10.0 speed cutoff 0.1 per frame; degenerate bones 0)" in out and "Smoothing Displacement" not in out
    z = np.load(path)
    want = {"pred", "covered", "spread", "recording", "frame_in_recording", "target", "stride", "blend", "frame_no", "online_lookahead",
            "pred_unsmoothed", "moved", "one_euro_cutoff", "one_euro_beta", "one_euro_dcutoff"}
    assert set(z.files) == want
    assert int(z["online_lookahead"]) == 2 and int(z["stride"]) == 3
    assert (float(z["one_euro_cutoff"]), float(z["one_euro_beta"]), float(z["one_euro_dcutoff"])) == EURO
    assert z["pred_unsmoothed"].shape == (F, 21, 3) and z["moved"].shape == (F,) and (z["covered"] == 0).sum() == 7 + 51
    # and they are what the in-process pass gives on the same tree, seed and nets
    _, a = run(world, 3, online=2, one_euro=EURO, metrics="full")
    assert a["pred"].tobytes() == z["pred"].tobytes() and a["pred_unsmoothed"].tobytes() == z["pred_unsmoothed"].tobytes()
