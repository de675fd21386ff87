"""Dense inference (`main.py --infer --dense`, not in the reference): dense_infer, whose docstring is the contract, the stages of its pass
(_dense_pass drives them; their figures land in ONE device log with named rows), and what Evaluator.eval_dense prints and writes."""
import os
import types

import numpy as np
import torch

from . import blocks, hip, ops, skeleton
from . import render as render_mod
from .config import IMU_NOISE_FLAGS
from .data import DenseWindows
from .evaluation import (METRICS, PCK_THRESHOLDS_CM, Breakdown, _accel_over_sequences, _error_summary, _jitter_imu, _jitter_pose,
                         aligned_summary, check_breakdown, imu_noise_key, imu_noise_line, pose_noise_key, pose_noise_line, print_aligned,
                         print_breakdown, print_reference)
from .train_step import call_upper

BLEND_SPACES, SMOOTH_TAPERS, FLOOR_MODES = ("joints", "bones", "rot"), ("box", "gauss"), ("measure", "clamp")
FLOOR_KEYS = ("foot_height_err_cm", "penetration_rate", "penetration_cm", "contact_precision", "contact_recall", "hover_cm")
FLOOR_TARGET_KEYS = ("target_penetration_rate", "target_penetration_cm", "target_contact_precision", "target_contact_recall")
DENSE_SAVED = ("pred", "covered", "spread", "recording", "frame_in_recording", "target")      # --save_pred: the per-frame arrays of the file
FIGURE_ROWS = ("blend", "spread", "single", "position", "bone_dev", "single_bone_dev", "rot_spread", "unsmoothed", "moved", "floor",
               "single_floor", "unclamped_floor", "unclamped")


def bone_lengths(bone_set):
    """L_b = float32(|body_b|), the norm taken in float64, of a bone set [20, 3] (row 0 of DenseWindows.src["skl"]): the lengths every
    predicted skeleton has, both nets placing a child at parent + q . body_b with q orthonormal.  -> (upper [14], lower [6])."""
    L = np.linalg.norm(np.asarray(bone_set, dtype=np.float64).reshape(-1, 3), axis=1).astype(np.float32)
    return L[list(skeleton.WALK_UPPER_ROWS)], L[list(skeleton.WALK_LOWER_ROWS)]


def smooth_weights(H, taper, who="smooth"):
    """The tap weights w[2 H + 1] (float32, k = -H .. H) of dense inference's temporal filter (ops.smooth_frames): "box" ones, "gauss"
    exp(-2 k^2 / H^2) -- a Gaussian of sigma H / 2, 0.135 at the window's ends -- computed in float64 and rounded once.  ``who``: the
    argument a refusal names."""
    if isinstance(H, bool) or not isinstance(H, (int, np.integer)) or not 1 <= H <= ops.SMOOTH_MAX_H:
        raise ValueError("%s: the half-width is an integer number of frames in [1, %d], got %r" % (who, ops.SMOOTH_MAX_H, H))
    if taper not in SMOOTH_TAPERS:
        raise ValueError("%s: taper %r is not one of %s" % (who, taper, ", ".join(SMOOTH_TAPERS)))
    k = np.arange(-int(H), int(H) + 1, dtype=np.float64)
    return (np.ones(len(k)) if taper == "box" else np.exp(-2.0 * k * k / float(H * H))).astype(np.float32)


def _check_smooth(smooth, who="smooth"):
    """smooth = (H, order, taper) of dense_infer (``who``: smooth or rot_smooth, the name a refusal carries), or None.  -> the tuple
    with plain ints."""
    if smooth is None:
        return None
    if not (isinstance(smooth, (tuple, list)) and len(smooth) == 3):
        raise ValueError("%s: (H, order, taper), got %r" % (who, smooth))
    H, order, taper = smooth
    smooth_weights(H, taper, who)
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 0 <= order <= 2:
        raise ValueError("%s: order (the polynomial's degree) is 0, 1 or 2, got %r" % (who, order))
    return int(H), int(order), taper


def _check_floor(floor):
    """floor = (mode, contact_cm, margin_cm) of dense_infer, or None.  -> (mode, contact height, margin), the two in plain floats."""
    if floor is None:
        return None
    if not (isinstance(floor, (tuple, list)) and len(floor) == 3):
        raise ValueError("floor: (mode, contact_cm, margin_cm), got %r" % (floor,))
    mode, contact_cm, margin_cm = floor
    if mode not in FLOOR_MODES:
        raise ValueError("floor: mode %r is not one of %s" % (mode, ", ".join(FLOOR_MODES)))
    for name, v, zero_ok in (("contact_cm", contact_cm, False), ("margin_cm", margin_cm, True)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0 or (v == 0 and not zero_ok):
            raise ValueError("floor: %s is a finite number of centimetres %s 0, got %r" % (name, ">=" if zero_ok else ">", v))
    return mode, float(contact_cm), float(margin_cm)


def _check_online(online, T=None):
    """online = L of dense_infer, the latency budget in frames, or None.  -> a plain int (T given: held to [0, T - 1])."""
    if online is None:
        return None
    if isinstance(online, bool) or not isinstance(online, (int, np.integer)) or online < 0 or (T is not None and online > T - 1):
        raise ValueError("online: the lookahead is an integer number of frames in [0, frame_no - 1]%s, got %r"
                         % ("" if T is None else " = [0, %d]" % (T - 1), online))
    return int(online)


def _check_one_euro(one_euro):
    """one_euro = (fc, beta, dc) of dense_infer, or None.  -> the tuple in plain floats."""
    if one_euro is None:
        return None
    if not (isinstance(one_euro, (tuple, list)) and len(one_euro) == 3):
        raise ValueError("one_euro: (fc, beta, dc), got %r" % (one_euro,))
    for name, v, low in (("fc (the minimum cutoff in cycles per frame)", one_euro[0], "> 0"), ("beta", one_euro[1], ">= 0"),
                         ("dc (the speed estimate's cutoff in cycles per frame)", one_euro[2], "> 0")):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0 or (v == 0 and low == "> 0"):
            raise ValueError("one_euro: %s is a finite number %s, got %r" % (name, low, v))
    return tuple(float(v) for v in one_euro)


def _check_render(render):
    """render = (directory, size, recordings_or_None, fps) of dense_infer, or None.  -> the tuple with plain values, the recordings a
    sorted tuple of distinct loader recording numbers."""
    if render is None:
        return None
    if not (isinstance(render, (tuple, list)) and len(render) == 4):
        raise ValueError("render: (directory, size, recordings or None, fps), got %r" % (render,))
    directory, size, recs, fps = render
    if not isinstance(directory, (str, os.PathLike)) or not str(directory):
        raise ValueError("render: the directory is a path, got %r" % (directory,))
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 64 <= size <= 1024 or size % 4:
        raise ValueError("render: size is a multiple of 4 in [64, 1024] pixels, got %r" % (size,))
    if isinstance(fps, bool) or not isinstance(fps, (int, np.integer)) or not 1 <= fps <= 100:
        raise ValueError("render: fps is an integer in [1, 100], got %r" % (fps,))
    if recs is not None:
        recs = list(recs)
        if not recs or any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 0 for r in recs):
            raise ValueError("render: recordings is None (all) or a non-empty list of loader recording numbers >= 0, got %r" % (render[2],))
        recs = tuple(sorted(set(int(r) for r in recs)))
    return os.fspath(directory), int(size), recs, int(fps)


def _floor_summary(sums, n, prefix="", target=False):
    """The floor figures from the column sums [22] of ops.floor_stats over ``n`` rows that count: every key of FLOOR_KEYS pooled over
    both feet under ``prefix`` + key, and per foot as a pair (joint 15, joint 19) under ``prefix`` + key + "_per_foot"; None where a
    denominator is 0.  ``target``: FLOOR_TARGET_KEYS as well, the recorded skeleton's own figures (never prefixed)."""
    s = np.asarray(sums, dtype=np.float64).reshape(2, 11)
    ratio = lambda a, b, scale=1.0: None if b == 0 else float(a) / float(b) * scale

    def figures(c, rows):
        out = {"foot_height_err_cm": ratio(c[0], rows, 100.0), "penetration_rate": ratio(c[2], rows), "penetration_cm": ratio(c[1], c[2], 100.0),
               "contact_precision": ratio(c[4], c[3]), "contact_recall": ratio(c[4], c[5]), "hover_cm": ratio(c[6], c[5], 100.0)}
        tgt = {"target_penetration_rate": ratio(c[8], rows), "target_penetration_cm": ratio(c[7], c[8], 100.0),
               "target_contact_precision": ratio(c[10], c[9]), "target_contact_recall": ratio(c[10], c[5])}
        return out, tgt

    pooled, feet = figures(s.sum(axis=0), 2 * n), [figures(s[k], n) for k in (0, 1)]
    res = {}
    for i, (keys, pre) in enumerate(((FLOOR_KEYS, prefix), (FLOOR_TARGET_KEYS, ""))[:2 if target else 1]):
        for k in keys:
            res[pre + k] = pooled[i][k]
            res[pre + k + "_per_foot"] = (feet[0][i][k], feet[1][i][k])
    return res


def dense_infer(base, imu_net, upper_net, lower_net, dataset, stride, blend="mean", batch_size=64, metrics="reference", blend_space=None,
                pose_noise=None, imu_noise=None, smooth=None, floor=None, rot_smooth=None, breakdown=None, render=None, online=None,
                one_euro=None):
    """Sliding-window inference over whole recordings (not in the reference): IMU -> Upper -> Lower over the overlapping windows of
    data.DenseWindows(dataset, stride, blend), in minibatches of ``batch_size`` windows exactly as _epoch_eval runs one (eval mode, no
    grad), every window's rows kept on the device; then every frame's pose is the weighted mean of the rows that cover it
    (mmego_blend_windows), and the reference's error kernels run on the blended frames and on the unblended window rows.
    -> (summary, arrays).  summary: all_cm, upper_cm, lower_cm, rot_deg, per_joint_cm of the blend as means over the covered frames; the
    same under single_ for the window rows; position_cm [T] the mean 21-joint error by position in the window (mmego_colsum_phase);
    spread_cm the mean disagreement of the windows about a frame; windows, frames, covered_frames, max_cover.  metrics="full": also
    aligned_summary's keys for the covered blended frames, with accel_cm taken PER RECORDING over its stitched blended frames (the first
    figure that sees window seams), and single_accel_cm for the stitched reference windows when stride == frame_no (else None).
    arrays (host): pred [F, 21, 3] (lower overwrites the shared hips; NaN where covered == 0), covered, spread, recording,
    frame_in_recording, target; the two nets' blended joints before assembly, upper [F, 15, 3] and lower [F, 8, 3] (zeros where uncovered);
    and, still on the device, win_up [W T, 45], win_lo [W T, 24] and the plan itself.
    blend_space: "joints" blends the 3-vectors of every joint independently (the launches above); "bones" blends every bone's DIRECTION
    over the cover, sets it to the body's bone length and walks the kinematic tree from the vector-blended roots (mmego_blend_bones with
    skeleton.WALK_UPPER / WALK_LOWER and bone_lengths of the campaign's bone set): the frames stay rigid skeletons, as every window's
    prediction is, and everything downstream runs on them unchanged.  None (the default) is "joints".  Given explicitly, either value
    adds to the summary bone_dev_cm, the mean over the covered frames and the 20 bones of | |bone| - L_b | on the blended rows (upper 14
    from the upper rows, lower 6 from the lower rows; mmego_bone_length_dev), single_bone_dev_cm, the same over the window rows,
    degenerate_bones, the bones that took mmego_blend_bones' fallback (0 for "joints"), and blend_space; and to the arrays fallback [F].
    "rot" blends in rotation space (mmego_blend_rot): both nets' rotations q and the head rotation R every row ran with (after any pose
    noise) are kept per window row, every bone's world rotation R^T q is averaged over the cover (the weighted chordal mean), and the
    nets' forward kinematics lays the rest bones of the campaign's bone set along the averages from the vector-blended roots -- rigid
    frames as under "bones", with the twist about every bone kept.  The summary gains rot_spread_deg, the mean over the covered frames
    of the windows' RMS rotational distance from the mean over the 14 upper bones, and degenerate_bones counts mmego_blend_rot's
    fallback; the arrays gain rot [F, 20, 4], the unit quaternions (w, x, y, z) of the blended WORLD rotations in BONES_ALL order (NaN
    where uncovered), rot_spread [F] in radians, bone_vectors [20, 3] -- pred's bones are rot applied to bone_vectors -- and, still on
    the device, win_q_up [W T, 14, 9], win_q_lo [W T, 6, 9] and win_R [W T, 9]; none of these is allocated in another space.  "rot"
    with smooth is refused (ValueError): the rotations would not be filtered with the positions; rot_smooth filters them.
    pose_noise=(deg, t, seed): every window row's head pose is perturbed before the nets see it (ops.pose_jitter), under ONE key for the
    whole pass (pose_noise_key(seed, 0, 0)) with the row's GLOBAL frame number (plan.row_frame) as its draw number: a frame carries one
    pose error in every window that serves it, as a per-frame estimator's error would, and the result does not depend on batch_size.
    imu_noise=(six sigmas, seed): every window row's IMU samples are perturbed before IMU_Net reads them (ops.imu_jitter), under ONE key
    for the whole pass (imu_noise_key(seed, 0, 0)) with the row's GLOBAL frame number (plan.row_frame) as row_ids and the plan's window
    number as win_ids: a frame keeps its white noise in every window that serves it, a bias belongs to its window -- overlapping windows
    see one frame under different offsets, as separately started estimators would -- and the result does not depend on batch_size.
    smooth=(H, order, taper): the pass's last stage, a zero-phase local-polynomial filter along time over every recording's stitched
    blended frames (ops.smooth_frames; under blend_space="bones" ops.smooth_bones with the walk tables and bone lengths of the blend, so
    the frames stay rigid): frame f becomes the value at f of the weighted least-squares polynomial of degree ``order`` (0, 1, 2) through
    the frames f - H .. f + H of its own recording, weights smooth_weights(H, taper); uncovered frames take no part and stay as they
    are.  Everything above then runs on the smoothed frames unchanged, and the blended frames' figures are kept beside them: the summary
    gains unsmoothed_all_cm, unsmoothed_upper_cm, unsmoothed_lower_cm, unsmoothed_rot_deg, unsmoothed_per_joint_cm (and
    unsmoothed_accel_cm under metrics="full"), moved_cm, the mean over the covered frames of the RMS distance over the upper joints that
    the filter moved a frame, smooth itself and smooth_fallback, the bones that kept their own frame's direction (0 in the column
    form); the arrays gain pred_unsmoothed [F, 21, 3] and moved [F].  None (the default): no launch, no key, the bytes of the pass
    without the argument.
    floor=(mode, contact_cm, margin_cm): the pass's notion of the ground, behind the blend and the filter.  Every frame's floor plane
    and contact flags come from the recording (DenseWindows.floor: the plane is given in the frame of the frame's own joints, so a
    joint's height is n . x + d), as the head pose does under --gt_head_pose.  mode "measure": ops.floor_stats on the final frames and
    on the window rows; the summary gains, pooled over both feet and as pairs (joint 15, joint 19) under key + "_per_foot",
    foot_height_err_cm (mean |h(prediction) - h(target)|), penetration_rate (feet under the plane per covered frame and foot),
    penetration_cm (the mean depth over the penetrating feet), contact_precision / contact_recall of "height < contact_cm" against the
    recorded flags, hover_cm (the mean height above the plane of the flagged feet), the same under single_ for the window rows, the
    recorded skeleton's own target_penetration_rate, target_penetration_cm, target_contact_precision, target_contact_recall (the noise
    floor of the plane fit), None where a denominator is 0, and floor itself; the arrays gain foot_height [F, 2] of the final frames
    (NaN where uncovered), ground [F, 4] and foot_contact [F, 2].  mode "clamp": ops.floor_clamp first raises every leg of the final
    lower frames whose foot or ankle lies under margin_cm, keeping the frame's own bone lengths; everything above then runs on the
    clamped frames, the frames before the clamp keep their figures under unclamped_ (the error figures and the floor figures; and
    unclamped_accel_cm under metrics="full"), the summary gains lift_cm (the mean lift over the lifted frames, None without one),
    lifted_frames and floor_fallback (the legs whose target was out of reach), the arrays pred_unclamped [F, 21, 3], lifted [F] and
    floor_fallback [F].  "clamp" under blend_space="rot" is refused (ValueError): the saved rotations would no longer produce pred.
    None (the default): no launch, no upload, no key, the bytes of the pass without the argument.
    rot_smooth=(H, order, taper), under blend_space="rot" only (ValueError in any other space): the filter along time in ROTATION
    space, behind the blend where smooth sits (ops.smooth_rot, once per net with the walk tables and rest bones of the blend).  With
    smooth's taps, weights and coefficients c_k, every bone's world rotation of frame f becomes the proper rotation nearest
    sum_k c_k A_k over the frames f - H .. f + H of its own recording -- at order 0 the weighted chordal mean of the neighbouring
    frames, at order 1 and 2 the local polynomial of the matrix entries projected onto the rotations -- the roots are filtered as
    smooth filters them, and the forward kinematics lays the rest bones along the filtered rotations: rigid frames, and rot applied to
    bone_vectors from pred's roots still gives pred.  Everything above then runs on the filtered frames unchanged (floor "measure"
    too; "clamp" and smooth stay refused under "rot").  The summary gains the unsmoothed_ figures and moved_cm as under smooth,
    rot_moved_deg, the mean over the covered frames of the RMS angle over the 14 upper bones that the filter turned a frame,
    rot_smooth itself, rot_smooth_fallback, the bones of both nets that kept their own frame's rotation, and rot_jitter_deg /
    unsmoothed_rot_jitter_deg: over the frames f whose neighbours f - 1, f + 1 are covered frames of the same recording and over the
    20 bones, the mean angle in degrees of D1^T D2 with D1 = Q_{f-1}^T Q_f and D2 = Q_f^T Q_{f+1} -- the rotational counterpart of
    the acceleration error, which needs no ground truth; computed on the host in float64 from the arrays' quaternions, None without
    such a frame.  The arrays gain pred_unsmoothed [F, 21, 3], rot_unsmoothed [F, 20, 4] (NaN where uncovered), moved [F] and rot_moved
    [F] in radians; rot and pred are the filtered ones.  None (the default): no launch, no allocation, no key, the bytes of the pass
    without the argument.
    breakdown=(bin_cm, nbins) (evaluation.BREAKDOWN_BINS is --breakdown's): the error of the FINAL frames -- behind blend, filter and
    clamp -- by action, by recording and as a distribution (evaluation.Breakdown's launches: mmego_colsum_groups over the per-frame
    error table, the group of a frame its action or its recording where covered != 0 and -1 elsewhere; mmego_hist_groups over the 21
    joint errors).  The summary gains evaluation.breakdown_summary's keys -- by_action, by_recording, percentiles_cm,
    percentile_clipped, beyond, per_joint_median_cm, pck_auc, breakdown; all group figures plain means over the group's covered frames,
    as this pass's own figures are; an action or a recording without a covered frame carries None -- and the arrays action [F] (int64,
    the number the frame's action directory is named by).  None (the default): no launch, no allocation, the bytes of the pass without
    the argument.
    render=(directory, size, recordings, fps): pictures of the FINAL frames -- behind blend, filter and clamp.  After the figures, every
    recording asked for (``recordings``: loader recording numbers, None for all; a number the loader does not have is refused) that has
    a covered frame is drawn on the device (render.render_frames: ops.render_prims and ops.render_raster, twice per chunk of frames) from
    what the pass holds in HBM -- the final frames, the targets, every frame's packed cloud and floor plane -- as ``size`` x 2 ``size``
    images, the front view left and the side view right, in the body-fixed camera of render.camera, and written as an animated PNG of
    ``fps`` frames per second, rec{recording:04d}_action{A}.png in ``directory`` (created; without the loader's rec_action_ the name
    ends behind the number), the recording's frames in order, an uncovered frame showing the target alone.  The summary gains
    rendered_recordings and rendered_frames; pred and every other array are untouched.  None (the default): no launch, no
    allocation, no key.
    online=L, an integer in [0, frame_no - 1]: what a RUNNING device could have answered L frames after the frame.  Frame f is blended
    from the windows that had ended by f + L alone (data.DensePlan's lookahead: the windows and every launch are those of the offline
    pass, only the cover is filtered; L = frame_no - 1 is the offline cover).  The first frame_no - 1 - L frames of every recording of
    at least frame_no frames are the WARM-UP, covered by nothing: they count as uncovered everywhere -- covered 0, pred NaN, segment
    -1, in no mean.  stride > L + 1 would leave later frames uncovered and is refused (ValueError), and so are smooth and rot_smooth,
    which read H frames ahead.  Everything else goes with it.  The summary gains online and warmup_frames.  None (the default): no
    key, the bytes of the pass without the argument.
    one_euro=(fc, beta, dc): the CAUSAL filter along time, where smooth sits -- behind the blend, in front of the floor clamp -- over
    every maximal stretch of covered frames of one recording (ops.one_euro_runs of the segments; ops.one_euro, under
    blend_space="bones" ops.one_euro_bones with the walk tables and bone lengths of the blend, so the frames stay rigid): the one-euro
    filter per joint, xhat_i = xhat_{i-1} + alpha(fc + beta |dhat_i|) (x_i - xhat_{i-1}) with dhat the filtered speed (cutoff dc) and
    alpha(c) = 2 pi c / (2 pi c + 1), all per frame; a stretch's first frame keeps its bytes, uncovered frames take no part.  It works
    with or without online and is refused with smooth, with rot_smooth and under blend_space="rot" (ValueError).  Everything above then
    runs on the filtered frames, and the blended frames keep their figures under unsmoothed_ exactly as under smooth (with
    unsmoothed_accel_cm under metrics="full"); the summary gains moved_cm, one_euro itself and one_euro_fallback, the bones that took
    their own frame's direction (0 in the column form); the arrays gain pred_unsmoothed [F, 21, 3] and moved [F].  None (the default):
    no launch, no allocation, no key, the bytes of the pass without the argument.
    The figures come down in one read (the histograms of breakdown in one more); the per-frame arrays in one each."""
    if metrics not in METRICS:
        raise ValueError("metrics: %r is not one of %s" % (metrics, ", ".join(METRICS)))
    if blend_space is not None and blend_space not in BLEND_SPACES:
        raise ValueError("blend_space: %r is not one of %s" % (blend_space, ", ".join(BLEND_SPACES)))
    smooth = _check_smooth(smooth)
    if blend_space == "rot" and smooth is not None:
        raise ValueError("smooth: the filter runs on joint positions, so under blend_space=\"rot\" the saved rotations would not be "
                         "filtered with them; rot_smooth filters the rotations along time and lays the positions along them")
    rot_smooth = _check_smooth(rot_smooth, "rot_smooth")
    if rot_smooth is not None and blend_space != "rot":
        raise ValueError("rot_smooth: the filter runs on the blended rotations, which only blend_space=\"rot\" keeps, got blend_space=%r; "
                         "smooth filters the positions of the other spaces" % (blend_space,))
    floor = _check_floor(floor)
    breakdown = check_breakdown(breakdown)
    render = _check_render(render)
    online, one_euro = _check_online(online, getattr(dataset, "frame_no", None)), _check_one_euro(one_euro)
    for name, given in (("smooth", smooth), ("rot_smooth", rot_smooth)):
        if online is not None and given is not None:
            raise ValueError("online: %s reads H frames ahead of the frame it writes, which is what online promises not to do; "
                             "one_euro filters along time without looking ahead" % name)
        if one_euro is not None and given is not None:
            raise ValueError("one_euro: it sits where %s sits, and one pass runs one filter along time" % name)
    if one_euro is not None and blend_space == "rot":
        raise ValueError("one_euro: the filter runs on joint positions, so under blend_space=\"rot\" the saved rotations would not be "
                         "filtered with them (a causal filter of rotations is not provided)")
    if online is not None and int(stride) > online + 1:
        raise ValueError("online: frame f is served by the windows that ended by f + %d, so a stride above %d leaves frames between "
                         "windows uncovered, got %r" % (online, online + 1, stride))
    if blend_space == "rot" and floor is not None and floor[0] == "clamp":
        raise ValueError("floor: the clamp moves joint positions, so under blend_space=\"rot\" the saved rotations would no longer "
                         "produce pred (with or without rot_smooth); \"measure\" goes with every space")
    plan = DenseWindows(dataset, base.device, stride, blend) if online is None else DenseWindows(dataset, base.device, stride, blend,
                                                                                                 lookahead=online)
    if breakdown is not None and plan.rec_action is None:
        raise ValueError("breakdown: the loader has no rec_action_ / rec_snippet_ (a data.PosePC has); there is nothing to group by")
    if plan.W == 0:
        raise ValueError("dense inference: no recording of %s has %d frames, so there is no window to run" % (dataset.root, plan.T))
    if render is not None:
        plan.ground()                  # (the pictures need every frame's plane: a loader without one is refused here, ahead of the pass)
    if render is not None and render[2] is not None and render[2][-1] >= len(plan.rec_off) - 1:
        raise ValueError("render: recording %d is not one of the loader's %d" % (render[2][-1], len(plan.rec_off) - 1))
    nets = [n for n in (imu_net, upper_net, lower_net) if n is not None]
    was_training = [n.training for n in nets]
    for n in nets:
        n.eval()
    try:
        opt = dict(metrics=metrics, blend_space=blend_space, smooth=smooth, floor=floor, pose_noise=pose_noise, imu_noise=imu_noise,
                   rot_smooth=rot_smooth, breakdown=breakdown, render=render)
        if online is not None:
            opt["online"] = online
        if one_euro is not None:
            opt["one_euro"] = one_euro
        return _dense_pass(base, plan, imu_net, upper_net, lower_net, int(batch_size), opt)
    finally:
        for n, tr in zip(nets, was_training):
            n.train(tr)


def figure_rows(T):
    """The device figure log's layout: row name -> row index, "position" -> the slice of its T rows (one per position in the window);
    T + 12 rows whichever options are on (a row whose option is off is neither written nor read); writers and readers index by name."""
    p = FIGURE_ROWS.index("position")
    return {name: slice(p, p + T) if i == p else i + (T - 1) * (i > p) for i, name in enumerate(FIGURE_ROWS)}


def _f32(dev, *shape):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _run_windows(base, plan, imu_net, upper_net, lower_net, batch_size, pose_noise, imu_noise, rot):
    """IMU -> Upper -> Lower over the plan's windows.  -> {win_up, win_lo}, every row on the device; ``rot``: and win_q_up, win_q_lo, win_R."""
    dev, W, T = base.device, plan.W, plan.T
    win = dict(win_up=_f32(dev, W * T, 45), win_lo=_f32(dev, W * T, 24))
    if rot:
        win.update(win_q_up=_f32(dev, W * T, 14, 9), win_q_lo=_f32(dev, W * T, 6, 9), win_R=_f32(dev, W * T, 9))
    state = {}
    if imu_noise is not None and imu_net is None:
        raise ValueError("imu_noise perturbs what IMU_Net reads: this pass takes the head pose from the recording")
    if imu_noise is not None:
        win_no = torch.arange(W, dtype=torch.int64, device=dev)                                        # [W]: the plan's window numbers
    if pose_noise is not None or imu_noise is not None:
        row_frame = torch.as_tensor(np.ascontiguousarray(plan.row_frame, dtype=np.int64)).to(dev)      # [W T]: every row's frame
    for s in range(0, W, batch_size):
        idx = np.arange(s, min(s + batch_size, W))
        b = plan.gather(idx)                                   # fresh copies: the nets transform `data` in place (Q1)
        B = len(idx)
        if B not in state:
            state[B] = (torch.zeros((6, B, 64), device=dev), torch.zeros((6, B, 64), device=dev))
        h0, c0 = state[B]
        tgt, body, imu = b["target"], b["skl"], b["imu"]
        if imu_noise is not None:
            imu = _jitter_imu(state, imu, imu_noise, imu_noise_key(imu_noise[1], 0, 0), row_ids=row_frame[s * T:(s + B) * T],
                              win_ids=win_no[s:s + B])
        R, t = base.head_pose(imu_net, imu, b["R_R0R"], tgt)
        if pose_noise is not None:
            R, t = _jitter_pose(state, R, t, pose_noise, pose_noise_key(pose_noise[2], 0, 0), ids=row_frame[s * T:(s + B) * T])
        up, q_up = call_upper(upper_net, b["data"], h0, c0, body, R, t)[:2]
        lo, q_lo = lower_net(up.clone(), b["data"], h0, h0, h0, h0, body, R, t)     # x already transformed once (Q1)
        rows = {"win_up": up, "win_lo": lo, "win_q_up": q_up, "win_q_lo": q_lo, "win_R": R}      # (R after any pose noise: what the row ran with)
        for name, dst in win.items():
            part = dst[s * T:(s + B) * T]
            part.copy_(rows[name].reshape(part.shape))
    return win


def _blend(plan, win, space):
    """Every frame from its windows.  -> up, lo, spread; a space: lengths; "bones", "rot": fell [2, F]; "rot": quat_*, rot_spread, bone_vectors."""
    dev, F, win_up, win_lo = plan.device, plan.F, win["win_up"], win["win_lo"]
    b = types.SimpleNamespace(up=_f32(dev, F, 45), lo=_f32(dev, F, 24), spread=_f32(dev, F),
                              fell=torch.zeros((2, F), dtype=torch.int32, device=dev) if space in ("bones", "rot") else None,
                              lengths=None if space is None else bone_lengths(plan.bone_set))
    if space == "bones":
        ops.blend_bones(win_up, plan, skeleton.WALK_UPPER, b.lengths[0], b.up, b.spread, b.fell[0])
        ops.blend_bones(win_lo, plan, skeleton.WALK_LOWER, b.lengths[1], b.lo, None, b.fell[1])
    elif space == "rot":
        b.quat_up, b.quat_lo, b.rot_spread = _f32(dev, F, 14, 4), _f32(dev, F, 6, 4), _f32(dev, F)
        body = b.bone_vectors = np.ascontiguousarray(np.asarray(plan.bone_set, dtype=np.float32).reshape(20, 3))
        ops.blend_rot(win_up, win["win_q_up"], win["win_R"], plan, skeleton.WALK_UPPER, skeleton.ROT_UPPER, body[list(skeleton.WALK_UPPER_ROWS)],
                      b.up, b.quat_up, b.spread, b.rot_spread, b.fell[0])
        ops.blend_rot(win_lo, win["win_q_lo"], win["win_R"], plan, skeleton.WALK_LOWER, skeleton.ROT_LOWER, body[list(skeleton.WALK_LOWER_ROWS)],
                      b.lo, b.quat_lo, None, None, b.fell[1])
    else:
        ops.blend_windows(win_up, plan, b.up, b.spread)
        ops.blend_windows(win_lo, plan, b.lo)
    return b


def _smooth(up, lo, seg, smooth, lengths):
    """The filter along time.  -> up, lo, moved [F], fell ([2, F] int32 in the bones form, ``lengths`` given; else None)."""
    (H, order, taper), dev, F = smooth, up.device, up.shape[0]
    wts = smooth_weights(H, taper)
    s = types.SimpleNamespace(up=_f32(dev, F, 45), lo=_f32(dev, F, 24), moved=_f32(dev, F), rot_moved=None,
                              fell=None if lengths is None else torch.zeros((2, F), dtype=torch.int32, device=dev))
    if lengths is not None:
        ops.smooth_bones(up, seg, wts, order, skeleton.WALK_UPPER, lengths[0], s.up, s.moved, s.fell[0])
        ops.smooth_bones(lo, seg, wts, order, skeleton.WALK_LOWER, lengths[1], s.lo, None, s.fell[1])
    else:
        ops.smooth_frames(up, seg, wts, order, s.up, s.moved)
        ops.smooth_frames(lo, seg, wts, order, s.lo)
    return s


def _one_euro(up, lo, plan, one_euro, lengths):
    """The causal filter along time.  -> up, lo, moved [F], fell ([2, F] int32 in the bones form, ``lengths`` given; else None)."""
    (fc, beta, dc), dev, F = one_euro, up.device, up.shape[0]
    runs = ops.one_euro_runs(np.where(plan.covered != 0, plan.frame_rec, -1).astype(np.int32))
    s = types.SimpleNamespace(up=_f32(dev, F, 45), lo=_f32(dev, F, 24), moved=_f32(dev, F), rot_moved=None, one_euro=True,
                              fell=None if lengths is None else torch.zeros((2, F), dtype=torch.int32, device=dev))
    if lengths is not None:
        ops.one_euro_bones(up, runs, fc, beta, dc, skeleton.WALK_UPPER, lengths[0], s.up, s.moved, s.fell[0])
        ops.one_euro_bones(lo, runs, fc, beta, dc, skeleton.WALK_LOWER, lengths[1], s.lo, None, s.fell[1])
    else:
        ops.one_euro(up, runs, fc, beta, dc, s.up, s.moved)
        ops.one_euro(lo, runs, fc, beta, dc, s.lo)
    return s


def _smooth_rot(b, seg, rot_smooth):
    """The filter along time in rotation space, on what _blend returned under "rot".  -> up, lo, quat_up, quat_lo, moved [F],
    rot_moved [F], fell [2, F] int32."""
    (H, order, taper), dev, F, body = rot_smooth, b.up.device, b.up.shape[0], b.bone_vectors
    wts = smooth_weights(H, taper, "rot_smooth")
    s = types.SimpleNamespace(up=_f32(dev, F, 45), lo=_f32(dev, F, 24), quat_up=_f32(dev, F, 14, 4), quat_lo=_f32(dev, F, 6, 4),
                              moved=_f32(dev, F), rot_moved=_f32(dev, F), fell=torch.zeros((2, F), dtype=torch.int32, device=dev))
    ops.smooth_rot(b.up, b.quat_up, seg, wts, order, skeleton.WALK_UPPER, body[list(skeleton.WALK_UPPER_ROWS)], s.up, s.quat_up, s.moved,
                   s.rot_moved, s.fell[0])
    ops.smooth_rot(b.lo, b.quat_lo, seg, wts, order, skeleton.WALK_LOWER, body[list(skeleton.WALK_LOWER_ROWS)], s.lo, s.quat_lo, None, None,
                   s.fell[1])
    return s


def rot_jitter_deg(quat, recording, covered):
    """The rotational jitter of quaternions quat [F, NB, 4] (w, x, y, z) along time, in degrees and float64: over the frames f whose
    neighbours f - 1 and f + 1 lie in the same recording, all three covered, and over the NB bones, the mean angle of D1^T D2 with
    D1 = Q_{f-1}^T Q_f and D2 = Q_f^T Q_{f+1}, Q the rotation of the normalised quaternion -- how much the frame-to-frame turn changes
    from one frame to the next.  None without such a frame.  Taken in quaternion algebra (a product of rotations is a product of unit
    quaternions, and the angle of d = (w, v) is 2 atan2(|v|, |w|), in [0, pi] whatever the sign of any quaternion): three products per
    frame and bone instead of three 3 x 3 matrix products."""
    rec, cov = np.asarray(recording), np.asarray(covered) != 0
    mid = np.flatnonzero(cov[1:-1] & cov[:-2] & cov[2:] & (rec[1:-1] == rec[:-2]) & (rec[1:-1] == rec[2:])) + 1
    if len(mid) == 0:
        return None
    q = np.ascontiguousarray(np.moveaxis(np.asarray(quat, dtype=np.float64), -1, 0))        # [4, F, NB]: a component is contiguous

    def conj_mul(a, b):                                            # conj(a) b: the quaternion of A^T B (up to the norms)
        (aw, ax, ay, az), (bw, bx, by, bz) = a, b
        return (aw * bw + ax * bx + ay * by + az * bz, aw * bx - ax * bw - ay * bz + az * by,
                aw * by + ax * bz - ay * bw - az * bx, aw * bz - ax * by + ay * bx - az * bw)
    step = conj_mul(q[:, :-1], q[:, 1:])                           # frame f to f + 1, once for every pair of neighbours
    dw, dx, dy, dz = conj_mul([c[mid - 1] for c in step], [c[mid] for c in step])
    # (the angle is homogeneous in d: the three quaternions' norms, 1 to float rounding, drop out of atan2's two arguments alike)
    ang = 2.0 * np.arctan2(np.sqrt(dx * dx + dy * dy + dz * dz), np.abs(dw))
    return float(np.degrees(ang).mean())


def _clamp(lo, ground, seg, margin):
    """The floor clamp on the lower rows.  -> lo, lifted [F], fell [F] int32."""
    dev, F = lo.device, lo.shape[0]
    c = types.SimpleNamespace(lo=_f32(dev, F, 24), lifted=_f32(dev, F), fell=torch.zeros(F, dtype=torch.int32, device=dev))
    ops.floor_clamp(lo, ground, seg, margin, c.lo, c.lifted, c.fell)
    return c


def _error_figures(up, lo, tgt, out):
    """The 43 column sums of mmego_pose_errors over rows with their targets, into the log row ``out``.  -> the per-row table."""
    E = _f32(tgt.device, tgt.shape[0], 43)
    hip.call("pose_errors", up, lo, tgt, tgt.shape[0], E)
    ops.colsum(E, out[:43])
    return E


def _floor_figures(lo, tgt, ground, contact, seg, H, out):
    """The column sums of ops.floor_stats over lower rows (a row whose seg is < 0 writes zeros), into the log row ``out``."""
    S = _f32(lo.device, lo.shape[0], ops.FLOOR_W)
    ops.floor_stats(lo, tgt, ground, contact, seg, H, S)
    ops.colsum(S, out[:ops.FLOOR_W])


def _accel_cm(up, lo, tgt, spans):
    """A frame set's acceleration error over its stitched recordings in cm (aligned_summary's mean); None without a span of 3 frames."""
    acc = _accel_over_sequences(tgt.device, up, lo, tgt, spans)
    return None if acc is None else float(np.mean(acc[None].mean(axis=1))) * 100


def _figures(plan, win, b, sm, cl, sets, seg, arrays, opt):
    """Every figure's launches into the named rows of ONE device log, its one device -> host read, and the summary read back under the
    same names.  b, sm, cl: what blend, filter and clamp returned (None: did not run); sets: the frame sets (up, lo) by their prefix."""
    dev, W, T, F, space, floor = plan.device, plan.W, plan.T, plan.F, opt["blend_space"], opt["floor"]
    win_up, win_lo, tgt_f, (up_f, lo_f) = win["win_up"], win["win_lo"], plan.src["target"], sets[""]
    cov = np.flatnonzero(plan.covered)
    Fc, cidx = len(cov), None if len(cov) == F else torch.as_tensor(cov).to(dev)
    # a per-frame tensor's covered rows (zero rows never enter a mean): the tensor itself when every frame is covered
    rows = lambda x: x.view(F, -1) if cidx is None else ops.gather_rows(x.view(F, -1), cidx, _f32(dev, Fc, x[0].numel()))
    full = opt["metrics"] == "full"
    WA = ops.pose_errors_aligned_width(21, len(PCK_THRESHOLDS_CM)) if full else 0
    row = figure_rows(T)
    bd, log_shape = None, (T + len(FIGURE_ROWS) - 1, max(43, WA))
    if opt.get("breakdown") is not None:                           # the grouped sums live behind the log, in the same buffer and read
        bd = Breakdown(opt["breakdown"], np.where(plan.covered != 0, plan.frame_rec, -1), plan.rec_action, plan.rec_snippet, full, dev)
        buf = torch.zeros(log_shape[0] * log_shape[1] + bd.floats(), dtype=torch.float32, device=dev)
        log = buf[:log_shape[0] * log_shape[1]].view(log_shape)
    else:
        log = torch.zeros(log_shape, dtype=torch.float32, device=dev)
    up_c, lo_c, tgt_c = rows(up_f), rows(lo_f), rows(tgt_f)
    E = _error_figures(up_c, lo_c, tgt_c, log[row["blend"]])
    ops.colsum(rows(b.spread), log[row["spread"], :1])
    row_idx = torch.as_tensor(plan.row_frame).to(dev)
    tgt_w = ops.gather_rows(tgt_f, row_idx, _f32(dev, W * T, 63))
    Ew = _error_figures(win_up, win_lo, tgt_w, log[row["single"]])
    ops.colsum_phase(Ew, T, log[row["position"], :43])
    if space is not None:
        D, Dw = _f32(dev, Fc, 20), _f32(dev, W * T, 20)
        for up, lo, dst in ((up_c, lo_c, D), (win_up, win_lo, Dw)):
            ops.bone_length_dev(up, skeleton.WALK_UPPER, b.lengths[0], dst[:, :14])
            ops.bone_length_dev(lo, skeleton.WALK_LOWER, b.lengths[1], dst[:, 14:])
        ops.colsum(D, log[row["bone_dev"], :20])
        ops.colsum(Dw, log[row["single_bone_dev"], :20])
    if space == "rot":
        ops.colsum(rows(b.rot_spread), log[row["rot_spread"], :1])
    if sm is not None:                                             # the frames before the filter, and how far it moved a frame
        _error_figures(rows(sets["unsmoothed_"][0]), rows(sets["unsmoothed_"][1]), tgt_c, log[row["unsmoothed"]])
        ops.colsum(rows(sm.moved), log[row["moved"], :1])
        if sm.rot_moved is not None:                               # (the rotation filter: the upper launch's mean turn beside it)
            ops.colsum(rows(sm.rot_moved), log[row["moved"], 1:2])
    if floor is not None:
        # the final frames, the window rows with their frames' planes and flags, the frames before the clamp (their upper rows: the final)
        Hc, (ground, contact) = floor[1] / 100.0, plan.floor()
        _floor_figures(lo_f, tgt_f, ground, contact, seg, Hc, log[row["floor"]])
        ground_w, contact_w = ops.gather_rows(ground, row_idx, _f32(dev, W * T, 4)), ops.gather_rows(contact, row_idx, _f32(dev, W * T, 2))
        _floor_figures(win_lo, tgt_w, ground_w, contact_w, torch.zeros(W * T, dtype=torch.int32, device=dev), Hc, log[row["single_floor"]])
        if cl is not None:
            _floor_figures(sets["unclamped_"][1], tgt_f, ground, contact, seg, Hc, log[row["unclamped_floor"]])
            _error_figures(up_c, rows(sets["unclamped_"][1]), tgt_c, log[row["unclamped"]])
    if full:
        thr = torch.tensor([c / 100.0 for c in PCK_THRESHOLDS_CM], dtype=torch.float32, device=dev)
        A, alog = _f32(dev, Fc, WA), torch.zeros(WA, dtype=torch.float32, device=dev)
        ops.pose_errors_aligned(up_c.view(Fc, 15, 3), lo_c.view(Fc, 8, 3), tgt_c.view(Fc, 21, 3), thr, A)
        ops.colsum(A, alog)
    if bd is not None:
        # the tables over ALL frames (an uncovered frame's row is in no group, whatever it holds): the ones above where every frame is covered
        if cidx is not None:
            E = _f32(dev, F, 43)
            hip.call("pose_errors", up_f, lo_f, tgt_f, F, E)
            if full:
                A = ops.pose_errors_aligned(up_f.view(F, 15, 3), lo_f.view(F, 8, 3), tgt_f.view(F, 21, 3), thr, _f32(dev, F, WA))
        hists = bd.launch(E, A if full else None, buf[log.numel():])
        host = buf.cpu().numpy().astype(np.float64)                # the figures' one device -> host read
        out, groups = host[:log.numel()].reshape(log_shape), bd.summary(host[log.numel():], hists.cpu().numpy())
    else:
        out = log.cpu().numpy().astype(np.float64)                 # the figures' one device -> host read
    s = _error_summary(out[row["blend"], :43], Fc)
    s.update(_error_summary(out[row["single"], :43], W * T, "single_"))
    s.update(position_cm=out[row["position"], :21].mean(axis=1) / W * 100, spread_cm=float(out[row["spread"], 0]) / Fc * 100, windows=W,
             frames=F, covered_frames=Fc, max_cover=plan.max_cover, stride=plan.stride, blend=plan.blend, frame_no=T)
    if opt.get("online") is not None:
        s.update(online=opt["online"], warmup_frames=plan.warmup)
    if space is not None:
        s.update(bone_dev_cm=float(out[row["bone_dev"], :20].mean()) / Fc * 100,
                 single_bone_dev_cm=float(out[row["single_bone_dev"], :20].mean()) / (W * T) * 100,
                 degenerate_bones=int(arrays["fallback"].sum()), blend_space=space)
    if space == "rot":
        s["rot_spread_deg"] = float(np.degrees(out[row["rot_spread"], 0] / Fc))
    if sm is not None:
        s.update(_error_summary(out[row["unsmoothed"], :43], Fc, "unsmoothed_"), moved_cm=float(out[row["moved"], 0]) / Fc * 100)
        fell = 0 if sm.fell is None else int(sm.fell.cpu().numpy().sum())
        if getattr(sm, "one_euro", False):
            s.update(one_euro=opt["one_euro"], one_euro_fallback=fell)
        elif sm.rot_moved is None:
            s.update(smooth=opt["smooth"], smooth_fallback=fell)
        else:
            s.update(rot_moved_deg=float(np.degrees(out[row["moved"], 1] / Fc)), rot_smooth=opt["rot_smooth"], rot_smooth_fallback=fell,
                     rot_jitter_deg=rot_jitter_deg(arrays["rot"], arrays["recording"], arrays["covered"]),
                     unsmoothed_rot_jitter_deg=rot_jitter_deg(arrays["rot_unsmoothed"], arrays["recording"], arrays["covered"]))
    if floor is not None:
        s.update(_floor_summary(out[row["floor"], :ops.FLOOR_W], Fc, target=True))
        s.update(_floor_summary(out[row["single_floor"], :ops.FLOOR_W], W * T, "single_"), floor=tuple(floor))
    if cl is not None:
        s.update(_floor_summary(out[row["unclamped_floor"], :ops.FLOOR_W], Fc, "unclamped_"))
        s.update(_error_summary(out[row["unclamped"], :43], Fc, "unclamped_"))
        lifted = arrays["lifted"]
        s.update(lift_cm=float(lifted[lifted > 0].astype(np.float64).mean()) * 100 if (lifted > 0).any() else None,
                 lifted_frames=int((lifted > 0).sum()), floor_fallback=int(arrays["floor_fallback"].sum()))
    if full:
        warm = 0 if opt.get("online") is None else T - 1 - opt["online"]                         # (online: behind the warm-up)
        spans = [(a + warm, e) for a, e in zip(plan.rec_off[:-1], plan.rec_off[1:]) if e - a >= T]      # the covered recordings, whole
        s.update(aligned_summary(np.concatenate([alog.cpu().numpy().astype(np.float64) / Fc, np.full(21, np.nan)])[None], 21))
        for prefix, (up, lo) in sets.items():                      # (accel_cm: per recording, not per minibatch)
            s[prefix + "accel_cm"] = _accel_cm(up, lo, tgt_f, spans)
        s["single_accel_cm"] = None
        if plan.stride == T:
            first = np.searchsorted(plan.recording, np.arange(len(plan.rec_off) - 1), side="left")
            last = np.searchsorted(plan.recording, np.arange(len(plan.rec_off) - 1), side="right")
            n_ref = (plan.rec_off[1:] - plan.rec_off[:-1]) // T
            acc = _accel_over_sequences(dev, win_up, win_lo, tgt_w, [((l - n) * T, l * T) for f, l, n in zip(first, last, n_ref) if l > f])
            s["single_accel_cm"] = None if acc is None else float(acc.mean()) * 100
    if bd is not None:
        s.update(groups)
    return s


def _assemble(cfg, upper, lower, covered):
    """pred [F, 21, 3] from host rows [F, 15, 3] and [F, 8, 3]: lower overwrites the shared hips (Demo_test.py:121-123), NaN uncovered."""
    pred = np.zeros((len(upper), 21, 3), dtype=np.float32)
    pred[:, list(cfg.upper_joint_map)] = upper
    pred[:, list(cfg.lower_joint_map)] = lower
    pred[covered == 0] = np.nan
    return pred


def _host_arrays(cfg, plan, win, b, sm, cl, sets, floor, breakdown=None):
    """dense_infer's arrays: every per-frame array down in one read, the window rows and the plan still on the device."""
    F, covered = plan.F, plan.covered
    host = lambda x, J: x.cpu().numpy().reshape(F, J, 3)
    up_h, lo_h = host(sets[""][0], 15), host(sets[""][1], 8)
    arrays = dict(pred=_assemble(cfg, up_h, lo_h, covered), covered=covered.astype(np.int32), spread=b.spread.cpu().numpy(),
                  recording=plan.frame_rec, frame_in_recording=plan.frame_in_recording,
                  target=plan.src["target"].cpu().numpy().reshape(F, 21, 3), upper=up_h, lower=lo_h, plan=plan, **win)
    if b.lengths is not None:                                      # (an explicit space; "joints" has no fallback: zeros)
        arrays["fallback"] = np.zeros(F, dtype=np.int32) if b.fell is None else b.fell.cpu().numpy().sum(axis=0, dtype=np.int32)
    if "win_R" in win:                                             # ("rot")
        def quats(q):                                              # [F, 20, 4] in BONES_ALL order
            q = np.concatenate([q.quat_up.cpu().numpy(), q.quat_lo.cpu().numpy()], axis=1)
            q[covered == 0] = np.nan
            return q
        arrays.update(rot=quats(b if sm is None else sm), rot_spread=b.rot_spread.cpu().numpy(), bone_vectors=b.bone_vectors)
    if sm is not None:
        arrays.update(pred_unsmoothed=_assemble(cfg, host(sets["unsmoothed_"][0], 15), host(sets["unsmoothed_"][1], 8), covered),
                      moved=sm.moved.cpu().numpy())
        if sm.rot_moved is not None:
            arrays.update(rot_unsmoothed=quats(b), rot_moved=sm.rot_moved.cpu().numpy())
    if floor is not None:
        ground, contact = (x.cpu().numpy() for x in plan.floor())
        arrays.update(foot_height=foot_heights(lo_h[:, [3, 7]], ground, covered != 0), ground=ground, foot_contact=contact)
    if cl is not None:
        arrays.update(pred_unclamped=_assemble(cfg, up_h, host(sets["unclamped_"][1], 8), covered), lifted=cl.lifted.cpu().numpy(),
                      floor_fallback=cl.fell.cpu().numpy())
    if breakdown is not None:
        arrays["action"] = plan.rec_action[plan.frame_rec]
    return arrays


def _render(plan, up, lo, render):
    """The pictures of the final frames (up [F, 45], lo [F, 24], on the device), one animated PNG per recording asked for that has a
    covered frame.  -> (recordings written, frames written)."""
    directory, size, recs, fps = render
    dev, F = plan.device, plan.F
    os.makedirs(directory, exist_ok=True)
    # the 21 joints of a frame from the two nets' rows, as _assemble lays them out (the lower rows own the shared hips): upper slots
    # 0..11 are the joints 0..11, slot 14 is joint 20; the lower slots 0..7 are the joints 12..19
    pred = _f32(dev, F, 63)
    ops.copy2d(up[:, :36], pred[:, :36])
    ops.copy2d(lo, pred[:, 36:60])
    ops.copy2d(up[:, 42:45], pred[:, 60:63])
    seg = torch.as_tensor(np.where(plan.covered != 0, plan.frame_rec, -1).astype(np.int32)).to(dev)
    ground, cloud, tgt = plan.ground(), plan.src["data"].view(F, plan.pc_no, 6), plan.src["target"]
    done = frames = 0
    for r in (range(len(plan.rec_off) - 1) if recs is None else recs):
        a, e = int(plan.rec_off[r]), int(plan.rec_off[r + 1])
        if e == a or not (plan.covered[a:e] != 0).any():
            continue
        img = render_mod.render_frames(pred[a:e], tgt[a:e], ground[a:e], cloud[a:e], seg[a:e], size)
        name = "rec%04d%s.png" % (r, "" if plan.rec_action is None else "_action%d" % plan.rec_action[r])
        render_mod.write_apng(os.path.join(directory, name), img.cpu().numpy(), fps)
        done, frames = done + 1, frames + (e - a)
    return done, frames


def _dense_pass(base, plan, imu_net, upper_net, lower_net, batch_size, opt):
    """dense_infer behind its argument checks: the nets are in eval mode.  opt: dense_infer's keywords from ``metrics`` on, by name."""
    space, smooth, floor, rot_smooth = opt["blend_space"], opt["smooth"], opt["floor"], opt["rot_smooth"]
    with torch.no_grad():
        win = _run_windows(base, plan, imu_net, upper_net, lower_net, batch_size, opt["pose_noise"], opt["imu_noise"], space == "rot")
        b = _blend(plan, win, space)
        sets, sm, cl, seg = {"": (b.up, b.lo)}, None, None, None   # the frame sets by the prefix of their figures: "" the final ones
        if smooth is not None or floor is not None or rot_smooth is not None:      # a covered frame's segment is its recording, an uncovered one has none
            seg = torch.as_tensor(np.where(plan.covered != 0, plan.frame_rec, -1).astype(np.int32)).to(base.device)
        if smooth is not None:
            sm = _smooth(b.up, b.lo, seg, smooth, b.lengths if space == "bones" else None)
            sets = {"": (sm.up, sm.lo), "unsmoothed_": sets[""]}
        if rot_smooth is not None:                                 # (never both: smooth is refused under "rot", rot_smooth elsewhere)
            sm = _smooth_rot(b, seg, rot_smooth)
            sets = {"": (sm.up, sm.lo), "unsmoothed_": sets[""]}
        if opt.get("one_euro") is not None:                        # (refused with either filter above)
            sm = _one_euro(b.up, b.lo, plan, opt["one_euro"], b.lengths if space == "bones" else None)
            sets = {"": (sm.up, sm.lo), "unsmoothed_": sets[""]}
        if floor is not None and floor[0] == "clamp":
            cl = _clamp(sets[""][1], plan.floor()[0], seg, floor[2] / 100.0)
            sets.update({"": (sets[""][0], cl.lo), "unclamped_": sets[""]})
        arrays = _host_arrays(base.cfg, plan, win, b, sm, cl, sets, floor, opt.get("breakdown"))
        summary = _figures(plan, win, b, sm, cl, sets, seg, arrays, opt)
        if opt.get("render") is not None:
            done, frames = _render(plan, sets[""][0], sets[""][1], opt["render"])
            summary.update(rendered_recordings=done, rendered_frames=frames)
    blocks.seq_xcd_raise()          # (the frozen IMU_Net's persistent launches: invalid head poses must not become a reported metric)
    return summary, arrays


def foot_heights(feet, ground, covered):
    """Heights [F, 2] (float32, from float64) of the feet [F, 2, 3] above the planes ground [F, 4], n . x + d with n normalised; NaN
    where ``covered`` is false or the plane has no normal (|n| <= 1e-6)."""
    g = np.asarray(ground, dtype=np.float64)
    norm = np.linalg.norm(g[:, :3], axis=1)
    ok = np.asarray(covered, dtype=bool) & (norm > 1e-6)
    safe = np.where(norm > 1e-6, norm, 1.0)
    h = (np.einsum("fki,fi->fk", np.asarray(feet, dtype=np.float64), g[:, :3]) + g[:, 3:4]) / safe[:, None]
    h[~ok] = np.nan
    return h.astype(np.float32)


def print_summary(s, opt, saved=None):
    """What `--infer --dense` prints: the reference's five lines first; ``saved``: where the per-frame skeletons were written."""
    space, smooth, floor, full = opt["blend_space"], opt["smooth"], opt["floor"], opt["metrics"] == "full"
    rot_smooth, online, one_euro = opt.get("rot_smooth"), opt.get("online"), opt.get("one_euro")
    print_reference(s)
    print("Single-window (unblended) Error(cm): all {} upper {} lower {} rotation(°) {}".format(
        s["single_all_cm"], s["single_upper_cm"], s["single_lower_cm"], s["single_rot_deg"]))
    print("Error by window position(cm): {}".format(s["position_cm"]))
    print("Window Disagreement(cm): {}".format(s["spread_cm"]))
    if space is not None:
        print("Bone Length Deviation(cm): blended {} single-window {} (degenerate bones {})".format(
            s["bone_dev_cm"], s["single_bone_dev_cm"], s["degenerate_bones"]))
    if space == "rot":
        print("Window Rotational Disagreement(°): {}".format(s["rot_spread_deg"]))
    if online is not None:
        print("Online: lookahead {} frames (frame f from the windows that ended by f + {}), warm-up frames {}".format(
            s["online"], s["online"], s["warmup_frames"]))
    print("Dense windows: {} windows of {} frames at stride {} (blend {}), {} of {} frames covered, largest cover {}{}".format(
        s["windows"], s["frame_no"], s["stride"], s["blend"], s["covered_frames"], s["frames"], s["max_cover"],
        "" if online is None else ", lookahead {}, warm-up frames {}".format(s["online"], s["warmup_frames"])))
    if full:
        print_aligned(s)
        print("Single-window Acceleration Error(cm/frame^2): {}".format(s["single_accel_cm"]))
    if saved:
        print("Per-frame skeletons saved in {}".format(saved))
    if opt["pose_noise"] is not None:
        print(pose_noise_line(opt["pose_noise"]))
    if opt["imu_noise"] is not None:
        print(imu_noise_line(opt["imu_noise"]))
    if smooth is not None:
        print("Unsmoothed (blended) Error(cm): all {} upper {} lower {} rotation(°) {}".format(
            s["unsmoothed_all_cm"], s["unsmoothed_upper_cm"], s["unsmoothed_lower_cm"], s["unsmoothed_rot_deg"]))
        print("Smoothing Displacement(cm): {} (window +-{} frames, order {}, {}; degenerate bones {})".format(
            s["moved_cm"], s["smooth"][0], s["smooth"][1], s["smooth"][2], s["smooth_fallback"]))
        if full:
            print("Unsmoothed Acceleration Error(cm/frame^2): {}".format(s["unsmoothed_accel_cm"]))
    if rot_smooth is not None:
        print("Unsmoothed (blended) Error(cm): all {} upper {} lower {} rotation(°) {}".format(
            s["unsmoothed_all_cm"], s["unsmoothed_upper_cm"], s["unsmoothed_lower_cm"], s["unsmoothed_rot_deg"]))
        print("Rotation Smoothing: displacement(cm) {} mean turn(°) {} (window +-{} frames, order {}, {}; degenerate bones {})".format(
            s["moved_cm"], s["rot_moved_deg"], s["rot_smooth"][0], s["rot_smooth"][1], s["rot_smooth"][2], s["rot_smooth_fallback"]))
        print("Rotational Jitter(°/frame^2): {} (blended {})".format(s["rot_jitter_deg"], s["unsmoothed_rot_jitter_deg"]))
        if full:
            print("Unsmoothed Acceleration Error(cm/frame^2): {}".format(s["unsmoothed_accel_cm"]))
    if floor is not None:
        print("Foot Height Error(cm): {} (joint 15: {}, joint 19: {}; single-window {})".format(
            s["foot_height_err_cm"], *s["foot_height_err_cm_per_foot"], s["single_foot_height_err_cm"]))
        print("Floor Penetration: rate {} depth(cm) {} (target: rate {} depth {}; single-window: rate {} depth {})".format(
            s["penetration_rate"], s["penetration_cm"], s["target_penetration_rate"], s["target_penetration_cm"],
            s["single_penetration_rate"], s["single_penetration_cm"]))
        print("Foot Contact by height < {:g} cm: precision {} recall {} (target: precision {} recall {})".format(
            floor[1], s["contact_precision"], s["contact_recall"], s["target_contact_precision"], s["target_contact_recall"]))
        print("Contact Hover(cm): {}".format(s["hover_cm"]))
        if floor[0] == "clamp":
            print("Unclamped Error(cm): all {} lower {} (penetration rate {} depth(cm) {})".format(
                s["unclamped_all_cm"], s["unclamped_lower_cm"], s["unclamped_penetration_rate"], s["unclamped_penetration_cm"]))
            print("Floor Clamp: {} of {} frames lifted, mean lift(cm) {}, unreachable legs {} (margin {:g} cm)".format(
                s["lifted_frames"], s["covered_frames"], s["lift_cm"], s["floor_fallback"], floor[2]))
    if opt.get("breakdown") is not None:
        print_breakdown(s)
    if opt.get("render") is not None:
        print("Rendered: {} recordings, {} frames -> {}".format(s["rendered_recordings"], s["rendered_frames"], opt["render"][0]))
    if one_euro is not None:
        print("Unsmoothed (blended) Error(cm): all {} upper {} lower {} rotation(°) {}".format(
            s["unsmoothed_all_cm"], s["unsmoothed_upper_cm"], s["unsmoothed_lower_cm"], s["unsmoothed_rot_deg"]))
        print("One-Euro Filter: displacement(cm) {} (min cutoff {} beta {} speed cutoff {} per frame; degenerate bones {})".format(
            s["moved_cm"], s["one_euro"][0], s["one_euro"][1], s["one_euro"][2], s["one_euro_fallback"]))
        if full:
            print("Unsmoothed Acceleration Error(cm/frame^2): {}".format(s["unsmoothed_accel_cm"]))


def saved_arrays(s, arrays, opt):
    """The dictionary `--save_pred` writes (np.savez): DENSE_SAVED and the plan's three settings, then what every option adds."""
    space, smooth, floor, rot_smooth = opt["blend_space"], opt["smooth"], opt["floor"], opt.get("rot_smooth")
    keep = lambda *names: {k: arrays[k] for k in names}
    d = dict(stride=np.int64(s["stride"]), blend=np.asarray(s["blend"]), frame_no=np.int64(s["frame_no"]), **keep(*DENSE_SAVED))
    if space is not None:
        d.update(blend_space=np.asarray(space), degenerate_bones=np.int64(s["degenerate_bones"]))
    if space == "rot":
        d.update(keep("rot", "rot_spread", "bone_vectors"))
    if smooth is not None:
        d.update(keep("pred_unsmoothed", "moved"), smooth_window=np.int64(smooth[0]), smooth_order=np.int64(smooth[1]),
                 smooth_taper=np.asarray(smooth[2]))
    if rot_smooth is not None:
        d.update(keep("pred_unsmoothed", "rot_unsmoothed", "moved", "rot_moved"), rot_smooth_window=np.int64(rot_smooth[0]),
                 rot_smooth_order=np.int64(rot_smooth[1]), rot_smooth_taper=np.asarray(rot_smooth[2]))
    if floor is not None:
        d.update(keep("foot_height", "ground", "foot_contact"), floor_mode=np.asarray(floor[0]), floor_contact_cm=np.float64(floor[1]),
                 floor_margin_cm=np.float64(floor[2]))
        if floor[0] == "clamp":
            d.update(keep("pred_unclamped", "lifted", "floor_fallback"))
    if opt["pose_noise"] is not None:
        deg, t, seed = opt["pose_noise"]
        d.update(pose_noise_deg=np.float64(deg), pose_noise_t=np.float64(t), pose_noise_seed=np.int64(seed))
    if opt["imu_noise"] is not None:
        d.update({flag: np.float64(v) for flag, v in zip(IMU_NOISE_FLAGS, opt["imu_noise"][0])}, imu_noise_seed=np.int64(opt["imu_noise"][1]))
    if opt.get("online") is not None:
        d["online_lookahead"] = np.int64(opt["online"])
    if opt.get("one_euro") is not None:
        fc, beta, dc = opt["one_euro"]
        d.update(keep("pred_unsmoothed", "moved"), one_euro_cutoff=np.float64(fc), one_euro_beta=np.float64(beta),
                 one_euro_dcutoff=np.float64(dc))
    if opt.get("breakdown") is not None:
        a, r = s["by_action"], s["by_recording"]
        nan = lambda x: np.asarray([np.nan if v is None else v for v in x], dtype=np.float64)
        d.update(keep("action"), by_action_action=np.asarray(a["action"], dtype=np.int64), by_action_frames=np.asarray(a["frames"], dtype=np.int64),
                 by_action_recordings=np.asarray(a["recordings"], dtype=np.int64),
                 **{"by_action_" + k: nan(a[k]) for k in a if k not in ("action", "frames", "recordings")},
                 by_recording_all_cm=nan(r["all_cm"]), by_recording_frames=np.asarray(r["frames"], dtype=np.int64),
                 error_hist=np.asarray(s["error_hist"], dtype=np.int64), error_hist_bin_cm=np.float64(s["breakdown"][0]))
    return d
