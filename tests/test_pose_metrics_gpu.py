"""GPU: the aligned evaluation metrics (csrc/metrics.hip: mmego_pose_errors_aligned, mmego_pose_accel_errors) against the float64
yardstick of tests/pose_metrics_ref.py (SVD / Umeyama: another method than the kernel's quaternion form), and processors.evaluate_full
with metrics="full" on the committed real sequences.

Bound on every output column: |out - ref| <= 2^-23 |ref| + 1e-7 -- the float store, and a floor two orders under the project's metric bar
(1e-3 cm = 1e-5 m) and eight above what the double computation leaves."""
import collections
import time

import numpy as np
import pytest
import torch

import pose_metrics_ref as ref
from conftest import golden, load_weights

pytestmark = pytest.mark.gpu

SENT = -12345.0
THR = np.array([0.05, 0.10, 0.15], dtype=np.float32)
KINDS = ("noisy", "mirrored", "similar", "identical")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _d(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def aligned(dev, upper, lower, target, thr=THR, pad=0):
    """One mmego_pose_errors_aligned launch on [F, ., 3] arrays -> float64 [F, width]; rows lda = width + pad apart in a buffer of
    sentinels with one more row behind the last: nothing but the width columns of the F rows is written."""
    from mmego_amd import hip
    F, J = upper.shape[0], 15 if lower is None else 21
    W = hip.lib().mmego_pose_errors_aligned_width(J, len(thr))
    assert W == 3 * J + 3 + len(thr)
    A = torch.full((F + 1, W + pad), SENT, dtype=torch.float32, device=dev)
    hip.call("pose_errors_aligned", _d(dev, upper), _d(dev, lower), _d(dev, target), F, _d(dev, thr) if len(thr) else None, len(thr), A, W + pad)
    out = A.cpu().numpy()
    assert np.all(out[:F, W:] == SENT) and np.all(out[F] == SENT)
    return out[:F, :W].astype(np.float64)


def accel(dev, upper, lower, target, pad=0):
    from mmego_amd import hip
    B, T, J = upper.shape[0], upper.shape[1], 15 if lower is None else 21
    Acc = torch.full((B + 1, J + pad), SENT, dtype=torch.float32, device=dev)
    hip.call("pose_accel_errors", _d(dev, upper), _d(dev, lower), _d(dev, target), B, T, Acc, J + pad)
    out = Acc.cpu().numpy()
    assert np.all(out[:B, J:] == SENT) and np.all(out[B] == SENT)
    return out[:B, :J].astype(np.float64)


def within(out, want):
    """-> the worst |out - want| in units of the bound 2^-23 |want| + 1e-7 (<= 1: inside)."""
    return float((np.abs(out - want) / (2.0 ** -23 * np.abs(want) + 1e-7)).max())


@pytest.mark.parametrize("J", [15, 21])
@pytest.mark.parametrize("F", [1, 127, 128, 129, 300])
def test_kernel_against_the_yardstick(dev, F, J):
    rng = np.random.default_rng(1000 * J + F)
    for kind in KINDS:
        p21, g, ang = ref.make_frames(kind, rng, F)
        up, lo = ref.split(p21, J)
        want = ref.aligned_rows(up, lo, g, THR)
        p, gg = ref.assemble(up, lo, g)
        absolute = (ref.joint_errors(p, gg) ** 2).sum(1)
        for pad in (0, 3):
            out = aligned(dev, up, lo, g, pad=pad)
            worst = within(out, want)
            print("F %d J %d %s lda width+%d: worst error / bound %.3f" % (F, J, kind, pad, worst))
            assert worst <= 1.0, (kind, pad, worst)
            rigid, sim = (out[:, J:2 * J] ** 2).sum(1), (out[:, 2 * J:3 * J] ** 2).sum(1)
            assert np.all(sim <= rigid + 1e-9) and np.all(rigid <= absolute + 1e-9), (kind, (sim - rigid).max(), (rigid - absolute).max())
            if kind == "identical":
                assert out[:, :3 * J].max() <= 1e-7 and out[:, 3 * J].max() <= 1e-3
            if kind == "similar":
                assert np.abs(out[:, 3 * J] - ang).max() <= 1e-3, np.abs(out[:, 3 * J] - ang).max()


@pytest.mark.parametrize("J", [15, 21])
@pytest.mark.parametrize("kind", ["collinear", "pred_point", "target_point"])
def test_degenerate_frames(dev, kind, J):
    """Where the best rotation is not unique any maximiser is accepted: the sums of squared residuals are what is unique."""
    rng = np.random.default_rng(2000 + J)
    F = 130
    p21, g, _ = ref.make_frames(kind, rng, F)
    up, lo = ref.split(p21, J)
    want = ref.aligned_rows(up, lo, g, THR)
    out = aligned(dev, up, lo, g)
    assert np.all(np.isfinite(out))
    assert within(out[:, :J], want[:, :J]) <= 1.0
    for name, c in (("rigid", slice(J, 2 * J)), ("similarity", slice(2 * J, 3 * J))):
        so, sw = (out[:, c] ** 2).sum(1), (want[:, c] ** 2).sum(1)
        print("%s J %d %s: worst sum e^2 error / (1e-6 max(1, ref)) %.3f" % (kind, J, name, (np.abs(so - sw) / (1e-6 * np.maximum(1.0, sw))).max()))
        assert np.all(np.abs(so - sw) <= 1e-6 * np.maximum(1.0, sw)), (name, np.abs(so - sw).max())
    if kind == "pred_point":
        assert np.all(out[:, 3 * J + 2] == 0.0) and np.all(out[:, 3 * J] == 0.0)
    assert within(out[:, 3 * J + 1:3 * J + 2], want[:, 3 * J + 1:3 * J + 2]) <= 1.0 and within(out[:, 3 * J + 3:], want[:, 3 * J + 3:]) <= 1.0


@pytest.mark.parametrize("J", [15, 21])
def test_invariances(dev, J):
    """No reference: a random similarity transform of the prediction leaves the similarity block where it was, a rigid one the rigid
    block, a shift the root-relative block, within the bound of the yardstick test (2^-23: two float stores).  The moved prediction is
    an fp32 input again, and its rounding is no property of the kernel: the skeletons here are the usual ones divided by 16 (exact in
    fp32; 2.5 cm wide, noise 3 mm, shifts of 2 cm), so every moved coordinate stays under 0.5 m, is rounded by at most 2^-26 m =
    1.5e-8 m, and moves a residual by at most that times sqrt(3) over the smallest scale 0.5 = 5.2e-8 m: half the bound's floor."""
    rng = np.random.default_rng(3000 + J)
    F = 200
    p21, g, _ = ref.make_frames("noisy", rng, F)
    p21, g = p21 / np.float32(16.0), g / np.float32(16.0)
    base = aligned(dev, *ref.split(p21, J), g)
    p64 = p21.astype(np.float64)
    moved = {"similarity": ref.similarity(rng, p64, shift=0.02)[0], "rigid": ref.similarity(rng, p64, scale=False, shift=0.02)[0],
             "shift": p64 + rng.normal(0.0, 0.02, (F, 1, 3))}
    for name, c in (("similarity", slice(2 * J, 3 * J)), ("rigid", slice(J, 2 * J)), ("shift", slice(0, J))):
        assert np.abs(moved[name]).max() < 0.5
        out = aligned(dev, *ref.split(moved[name].astype(np.float32), J), g)
        worst = within(out[:, c], base[:, c])
        print("J %d %s: worst difference / bound %.3f" % (J, name, worst))
        assert worst <= 1.0, (name, worst)


def test_pck_on_the_committed_metric_fixture(dev):
    g8 = golden("g8_metric.npz")
    pred, target = g8["pred"].reshape(-1, 21, 3).astype(np.float32), g8["target"].reshape(-1, 21, 3).astype(np.float32)
    err = ref.joint_errors(pred.astype(np.float64), target.astype(np.float64))
    assert err.size == 420
    gaps = [float(np.abs(err - float(t)).min()) for t in (0.05, 0.10, 0.15)]
    print("smallest distance of a joint error from each threshold:", gaps)
    assert min(gaps) >= 1e-6
    up, lo = ref.split(pred, 21)
    out = aligned(dev, up, lo, target)[:, 66:]
    want = ref.pck(pred.astype(np.float64), target.astype(np.float64), THR)
    assert out.shape == want.shape == (20, 3) and np.abs(out - want).max() <= 1e-6
    assert np.abs(out.mean(0) - (err[..., None] <= THR.astype(np.float64)).mean((0, 1))).max() <= 1e-6
    # the 15 upper joints, and a launch without thresholds
    out15 = aligned(dev, up, None, target)[:, 48:]
    assert np.abs(out15 - ref.pck(*ref.assemble(up, None, target), THR)).max() <= 1e-6
    assert aligned(dev, up, lo, target, thr=THR[:0]).shape == (20, 66)


@pytest.mark.parametrize("J", [15, 21])
@pytest.mark.parametrize("B,T", [(1, 3), (2, 4), (3, 20)])
def test_acceleration_kernel(dev, B, T, J):
    rng = np.random.default_rng(4000 + 100 * B + T + J)
    p21, g, _ = ref.make_frames("noisy", rng, B * T)
    p21 = p21 + rng.normal(0.0, 0.02, p21.shape).astype(np.float32)
    up, lo = ref.split(p21.reshape(B, T, 21, 3), J)
    g = g.reshape(B, T, 21, 3)
    want = ref.accel_errors(up, lo, g)
    for pad in (0, 3):
        worst = within(accel(dev, up, lo, g, pad), want)
        print("B %d T %d J %d lda J+%d: worst error / bound %.3f" % (B, T, J, pad, worst))
        assert worst <= 1.0


def test_bad_arguments_raise(dev):
    from mmego_amd import hip
    rng = np.random.default_rng(5)
    p21, g, _ = ref.make_frames("noisy", rng, 4)
    up, lo = ref.split(p21, 21)
    a = lambda x: _d(dev, x)
    Acc = torch.zeros((2, 21), device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("pose_accel_errors", a(up), a(lo), a(g), 2, 2, Acc, 21)                      # T = 2
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("pose_accel_errors", a(up), a(lo), a(g), 1, 4, Acc, 20)                      # lda < J
    A = torch.zeros((4, 80), device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("pose_errors_aligned", a(up), a(lo), a(g), 4, a(THR), 3, A, 68)              # lda < width
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("pose_errors_aligned", a(up), a(lo), a(g), 4, a(THR), 9, A, 80)              # nthr > 8
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("pose_errors_aligned", a(up), a(lo), a(g), 4, None, 3, A, 80)                # thresholds missing
    assert float(A.abs().max()) == 0.0 and float(Acc.abs().max()) == 0.0                     # nothing was launched


def test_two_launches_are_bit_equal(dev):
    rng = np.random.default_rng(6)
    p21, g, _ = ref.make_frames("mirrored", rng, 300)
    for J in (15, 21):
        up, lo = ref.split(p21, J)
        assert np.array_equal(aligned(dev, up, lo, g), aligned(dev, up, lo, g))
        s = lambda x: None if x is None else x.reshape(15, 20, -1, 3)
        assert np.array_equal(accel(dev, s(up), s(lo), s(g)), accel(dev, s(up), s(lo), s(g)))


def _mean_of_minibatch_means(rows):
    return np.mean(np.stack(rows), axis=0)


def test_evaluate_full_with_all_metrics_on_real_sequences(dev, real16, monkeypatch):
    """processors.evaluate_full(metrics="full") on the 16 committed sequences (pretrained goldens, recorded head pose; one sequence per
    minibatch, what --infer runs): the reference's tuple and summary keys bit for bit those of metrics="reference", the new keys
    within 1e-3 cm (the project's metric bar; the angle 1e-2 deg, as rot_deg) of the yardstick applied to the very tensors the two new
    launches were handed and averaged by the same convention; metrics="reference" launches neither new entry point."""
    from mmego_amd import hip, nets, processors
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import ArraySplit
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    up = load_weights(nets.UpperNet(), golden("w_upper_pretrained.npz")).to(dev).eval()
    lo = load_weights(nets.LowerNet(64), golden("w_lower_pretrained.npz")).to(dev).eval()
    split = ArraySplit(real16["x"], real16["target"], real16["skl"], real16["imu"], real16["R"])
    launches, seen = [], []
    real_call = hip.call

    def recording(name, *args):
        launches.append(name)
        if name in ("pose_errors_aligned", "pose_accel_errors"):
            seen.append((name, [None if a is None else a.detach().cpu().numpy().copy() for a in args[:3]]))
        return real_call(name, *args)

    monkeypatch.setattr(hip, "call", recording)
    t0 = time.time()
    out_ref, s_ref = processors.evaluate_full(base, None, up, lo, split, 1, False)
    assert "pose_errors_aligned" not in launches and "pose_accel_errors" not in launches and "pose_errors" in launches
    del launches[:]
    out_full, s_full = processors.evaluate_full(base, None, up, lo, split, 1, False, metrics="full")
    with_option = collections.Counter(launches)
    del launches[:]
    out_again, s_again = processors.evaluate_full(base, None, up, lo, split, 1, False)     # (as warm as the pass before it: same one-time work done)
    print("three passes: %.2f s" % (time.time() - t0))
    without = collections.Counter(launches)
    assert "pose_errors_aligned" not in without and "pose_accel_errors" not in without
    # each new launch and its colsum per minibatch, nothing else, nothing less
    assert with_option - without == collections.Counter({"pose_errors_aligned": 16, "pose_accel_errors": 16, "colsum": 32}) and not without - with_option
    for a, b in zip(out_ref, out_again):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(out_ref, out_full):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert set(s_ref) == {"all_cm", "upper_cm", "lower_cm", "rot_deg", "per_joint_cm"}
    for k in s_ref:
        assert np.array_equal(np.asarray(s_ref[k]), np.asarray(s_full[k])), k
    # the yardstick on what the launches were handed
    rows = [ref.aligned_rows(a[0], a[1], a[2], THR).mean(axis=0) for n, a in seen if n == "pose_errors_aligned"]
    accs = [ref.accel_errors(a[0], a[1], a[2]).mean(axis=0) for n, a in seen if n == "pose_accel_errors"]
    assert len(rows) == 16 and len(accs) == 16 and all(a[0].shape == (1, 20, 15, 3) and a[1].shape == (1, 20, 8, 3) for _, a in seen)
    m, acc = np.stack(rows), np.stack(accs)
    J, um, lm = 21, ref.UPPER_MAP, ref.LOWER_MAP
    want = {"align_rot_deg": m[:, 63].mean(), "align_shift_cm": m[:, 64].mean() * 100, "pa_scale": m[:, 65].mean(),
            "accel_cm": acc.mean(axis=1).mean() * 100}
    for name, c in (("root_rel", 0), ("rigid", J), ("pa", 2 * J)):
        blk = m[:, c:c + J]
        want[name + "_cm"] = blk.mean(axis=1).mean() * 100
        want[name + "_upper_cm"] = blk[:, um].mean(axis=1).mean() * 100
        want[name + "_lower_cm"] = blk[:, lm].mean(axis=1).mean() * 100
    for k, v in want.items():
        tol = 1e-2 if k == "align_rot_deg" else 1e-3
        print("%s: %.6f (yardstick %.6f)" % (k, s_full[k], v))
        assert abs(s_full[k] - v) <= tol, (k, s_full[k], v)
    assert set(s_full["pck"]) == set(processors.PCK_THRESHOLDS_CM)
    for i, c in enumerate(processors.PCK_THRESHOLDS_CM):
        assert abs(s_full["pck"][c] - m[:, 66 + i].mean()) <= 1e-6, c
    assert np.abs(s_full["per_joint_root_rel_cm"] - m[:, :J].mean(axis=0) * 100).max() <= 1e-3
    assert np.abs(s_full["per_joint_pa_cm"] - m[:, 2 * J:3 * J].mean(axis=0) * 100).max() <= 1e-3
    assert set(s_full) == set(s_ref) | set(want) | {"pck", "per_joint_root_rel_cm", "per_joint_pa_cm"}


def test_upper_stage_evaluation_with_all_metrics(dev, real16):
    """UpperTrainer.eval_model with metrics="full" (minibatches of 5, 5, 5 and 1 sequences, shuffled): the reference's six values bit
    for bit, the 15-joint summary on last_metrics."""
    from mmego_amd import nets, processors
    from mmego_amd.config import Config
    from mmego_amd.data import ArraySplit
    Config.gt_head_pose = True
    outs = {}
    for metrics in ("reference", "full"):
        Config.metrics = metrics
        try:
            base = processors._Base(Config, make_dirs=False)
            base.model = load_weights(nets.UpperNet(), golden("w_upper_pretrained.npz")).to(dev)
            base.model_IMU, base.batchsize = None, 5
            base.test_data = ArraySplit(real16["x"], real16["target"], real16["skl"], real16["imu"], real16["R"])
            base._rng = np.random.RandomState(77)
            outs[metrics] = (processors.UpperTrainer.eval_model(base), base.last_metrics)
        finally:
            Config.metrics = "reference"
    for a, b in zip(outs["reference"][0], outs["full"][0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    s = outs["full"][1]
    assert outs["reference"][1] is None and "root_rel_upper_cm" not in s and s["per_joint_pa_cm"].shape == (15,)
    assert s["pa_cm"] > 0.0 and s["rigid_cm"] > 0.0 and s["root_rel_cm"] > 0.0 and s["accel_cm"] > 0.0 and 0.0 <= s["pck"][5.0] <= s["pck"][15.0] <= 1.0
    assert "PA-MPJPE" in processors.metrics_line(s)
