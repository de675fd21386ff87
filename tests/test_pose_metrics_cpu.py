"""CPU (no GPU): the float64 yardstick of the aligned evaluation metrics (tests/pose_metrics_ref.py) against an independent second
formulation and under the invariances its definition implies; the parser's refusals of --metrics; the host-only width helper."""
import os
import sys

import numpy as np
import pytest

import pose_metrics_ref as ref
from conftest import ROOT


@pytest.mark.parametrize("kind", ["noisy", "mirrored", "similar"])
@pytest.mark.parametrize("J", [15, 21])
def test_svd_yardstick_equals_the_quaternion_formulation(kind, J):
    """Umeyama's SVD solution with the determinant correction and Horn's quaternion form through numpy.linalg.eigh share no step behind
    the cross-covariance; on seeded skeletons whose best rotation is unique they give the same residuals, angle and scale."""
    rng = np.random.default_rng(100 + J)
    p21, g, _ = ref.make_frames(kind, rng, 500)
    p, g = ref.assemble(*ref.split(p21, J), g)
    a, b = ref.fit_errors(p, g, ref.umeyama_fit), ref.fit_errors(p, g, ref.horn_fit)
    for name, x, y, tol in (("rigid", a[0], b[0], 1e-12), ("similarity", a[1], b[1], 1e-12), ("angle", a[2], b[2], 1e-9),
                            ("scale", a[4], b[4], 1e-12)):
        assert np.abs(x - y).max() <= tol, (kind, name, np.abs(x - y).max())
    R, _ = ref.umeyama_fit(p, g)
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-12                       # proper rotations, the mirrored skeletons included
    if kind == "similar":
        assert a[1].max() < 2e-6 and np.abs(a[4] * ref.fit_errors(g, p)[4] - 1.0).max() < 1e-6     # (fp32 inputs: exact up to their rounding)


def test_yardstick_on_degenerate_frames():
    """Where the rotation is not unique the sum of squared residuals still is: both formulations agree on it; defined values otherwise."""
    rng = np.random.default_rng(7)
    for kind in ("collinear", "pred_point", "target_point", "identical"):
        p21, g, _ = ref.make_frames(kind, rng, 200)
        p, g = ref.assemble(*ref.split(p21, 21), g)
        a, b = ref.fit_errors(p, g, ref.umeyama_fit), ref.fit_errors(p, g, ref.horn_fit)
        for i in (0, 1):
            sa, sb = (a[i] ** 2).sum(1), (b[i] ** 2).sum(1)
            assert np.all(np.isfinite(sa)) and np.abs(sa - sb).max() <= 1e-12 * max(1.0, sa.max()), (kind, i)
        if kind == "pred_point":
            assert np.all(a[4] == 0.0) and np.all(a[2] == 0.0)
        if kind == "identical":
            assert a[0].max() < 1e-12 and a[1].max() < 1e-12 and a[2].max() < 1e-6 and np.abs(a[4] - 1.0).max() < 1e-12


def test_yardstick_invariances():
    """The similarity residuals do not change when the prediction goes through a similarity transform, the rigid ones under a rigid
    transform, the root-relative errors under a shift (float64 inputs: no rounding of the transformed prediction)."""
    rng = np.random.default_rng(11)
    p21, g, _ = ref.make_frames("noisy", rng, 300)
    p, g = p21.astype(np.float64), g.astype(np.float64)
    base = ref.fit_errors(p, g)
    assert np.abs(ref.fit_errors(ref.similarity(rng, p)[0], g)[1] - base[1]).max() < 1e-12
    assert np.abs(ref.fit_errors(ref.similarity(rng, p, scale=False)[0], g)[0] - base[0]).max() < 1e-12
    assert np.abs(ref.root_relative(p + rng.normal(size=(300, 1, 3)), g) - ref.root_relative(p, g)).max() < 1e-12
    # and the fit never loses against doing nothing, nor the similarity fit against the rigid one
    ab = (ref.joint_errors(p, g) ** 2).sum(1)
    assert np.all((base[1] ** 2).sum(1) <= (base[0] ** 2).sum(1) + 1e-12) and np.all((base[0] ** 2).sum(1) <= ab + 1e-12)


def test_pck_and_acceleration_error_by_hand():
    g = np.zeros((1, 4, 21, 3))
    p = np.zeros((1, 4, 21, 3))
    p[0, :, 3, 0] = [0.0, 0.06, 0.0, 0.0]                    # joint 3 jumps by 6 cm in frame 1
    up, lo = ref.split(p, 21)
    assert np.allclose(ref.pck(*ref.assemble(up[0], lo[0], g[0]), [0.05, 0.10])[1], [20.0 / 21.0, 1.0])
    acc = ref.accel_errors(up, lo, g)
    assert acc.shape == (1, 21) and np.isclose(acc[0, 3], (0.12 + 0.06) / 2) and acc[0, :3].max() == 0.0
    acc15 = ref.accel_errors(up, None, g)
    assert acc15.shape == (1, 15) and np.isclose(acc15[0, 3], 0.09)
    rows = ref.aligned_rows(up[0], lo[0], g[0], [0.05])
    assert rows.shape == (4, 3 * 21 + 3 + 1) and np.isclose(rows[1, 3], 0.06) and rows[0].max() == 1.0      # (frame 0: only its PCK is not 0)


def _parse(argv):
    sys.path.insert(0, ROOT)
    import main
    parser = main.build_parser()
    args = parser.parse_args(argv)
    main.check_finetune(parser, args, 1)
    return args


def test_metrics_flag_is_accepted_where_skeletons_are_evaluated():
    assert _parse(["--infer"]).metrics == "reference"
    assert _parse(["--infer", "--metrics", "full"]).metrics == "full"
    for net in ("Upper_Net", "Lower_Net"):
        assert _parse(["--train", "--network", net, "--metrics", "full"]).metrics == "full"
    assert _parse(["--train", "--network", "IMU_Net", "--metrics", "reference"]).metrics == "reference"


@pytest.mark.parametrize("argv,needle", [
    (["--train", "--network", "IMU_Net", "--metrics", "full"], "does not go with --network IMU_Net"),
    (["--metrics", "full"], "goes with --train or --infer"),
    (["--network", "Upper_Net", "--metrics", "full"], "goes with --train or --infer"),
])
def test_metrics_flag_refusals(argv, needle, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2 and needle in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse(["--infer", "--metrics", "everything"])


def test_summary_of_the_extra_log_columns():
    """processors.aligned_summary on hand-made per-minibatch means (two minibatches): means over minibatches, cm, the upper / lower
    means over the joint maps for J = 21 only, PCK by threshold, and accel_cm None where no acceleration error was taken (T < 3)."""
    from mmego_amd import processors
    for J in (15, 21):
        m = np.zeros((2, 3 * J + 3 + 3 + J))
        m[0, :J], m[1, :J] = 0.01, 0.03                       # root-relative: 1 cm and 3 cm
        m[:, 2 * J + 12] = 0.21                               # one joint of the similarity block (joint 12: upper AND lower map)
        m[:, 3 * J], m[:, 3 * J + 1], m[:, 3 * J + 2] = 4.0, 0.5, 0.9
        m[:, 3 * J + 3:3 * J + 6] = (0.25, 0.5, 1.0)
        m[:, 3 * J + 6:] = 0.002
        s = processors.aligned_summary(m, J)
        assert np.isclose(s["root_rel_cm"], 2.0) and np.isclose(s["pa_cm"], 21.0 / J) and s["rigid_cm"] == 0.0
        assert (s["align_rot_deg"], s["pa_scale"]) == (4.0, 0.9) and np.isclose(s["align_shift_cm"], 50.0)
        assert s["pck"] == {5.0: 0.25, 10.0: 0.5, 15.0: 1.0} and np.isclose(s["accel_cm"], 0.2)
        assert s["per_joint_pa_cm"].shape == (J,) and np.isclose(s["per_joint_pa_cm"][12], 21.0) and np.allclose(s["per_joint_root_rel_cm"], 2.0)
        assert ("pa_upper_cm" in s) == (J == 21)
        if J == 21:
            assert np.isclose(s["pa_upper_cm"], 21.0 / 15) and np.isclose(s["pa_lower_cm"], 21.0 / 8) and np.isclose(s["root_rel_lower_cm"], 2.0)
        m[:, 3 * J + 6:] = np.nan
        assert processors.aligned_summary(m, J)["accel_cm"] is None
        assert "n/a" in processors.metrics_line(processors.aligned_summary(m, J)) and "PA-MPJPE" in processors.metrics_line(s)


def test_row_width_helper_and_thresholds():
    """mmego_pose_errors_aligned_width is a pure host function: safe without a GPU."""
    from mmego_amd import build, hip, processors
    build.build_library()
    w = hip.lib().mmego_pose_errors_aligned_width
    assert (w(21, 3), w(15, 0), w(15, 8)) == (69, 48, 56)
    assert processors.PCK_THRESHOLDS_CM == (5.0, 10.0, 15.0) and processors.METRICS == ("reference", "full")
    assert [n for _, n in hip.parse_header()["mmego_pose_accel_errors"]] == ["stream", "upper", "lower", "target", "B", "T", "Acc", "lda"]
    assert os.path.exists(os.path.join(ROOT, "mmego_amd", "csrc", "metrics.hip"))
