"""What processors._epoch_eval / evaluate_full and dense.dense_infer share: option names, noise keys and launches, figures, printed lines."""
import numpy as np
import torch

from . import ops
from .config import IMU_NOISE_FLAGS, Config
from .data import _mix64

METRICS = ("reference", "full")                                          # --metrics
PCK_THRESHOLDS_CM = (5.0, 10.0, 15.0)                                    # --metrics full: PCK of the absolute joint errors
POSE_NOISE_SALT = 0x504F5345                                             # the head-pose draws' stream among what _mix64 derives from --seed
IMU_NOISE_SALT = 0x494D554E                                              # the IMU draws' stream among what _mix64 derives from --seed


def pose_noise_key(seed, epoch, minibatch, rank=None):
    """The key of one minibatch's head-pose draw (--pose_noise_deg / --pose_noise_t): a pure function of (seed, epoch, minibatch number
    [, rank]), so --resume continues the sequence with no saved state and the ranks of a data-parallel run draw differently.  rank None:
    the evaluation passes' key, which has no rank.  -> the 63 bits mmego_pose_jitter's int64 device word takes."""
    words = (int(seed), int(epoch), int(minibatch)) + (() if rank is None else (int(rank),))
    return _mix64(*words, POSE_NOISE_SALT) & 0x7FFFFFFFFFFFFFFF


def pose_noise_of(cfg):
    """(deg, t, seed) of a run's --pose_noise_deg / --pose_noise_t (a missing sigma: 0.0; a missing --seed: 0, as --point_noise treats
    it), or None without the flags."""
    deg, t = getattr(cfg, "pose_noise_deg", None), getattr(cfg, "pose_noise_t", None)
    if deg is None and t is None:
        return None
    return (0.0 if deg is None else float(deg), 0.0 if t is None else float(t), int(getattr(cfg, "seed", None) or 0))


def pose_noise_line(pose_noise):
    return "Head Pose Noise: rotation {} deg per axis, translation {} m, seed {}".format(*pose_noise)


def _jitter_pose(scratch, R, t, pose_noise, key, ids=None):
    """An evaluation minibatch's head pose perturbed out of place (buffers and the device word kept in ``scratch`` per shape)."""
    R, t = R.contiguous(), t.contiguous()
    slot = ("pose_noise",) + tuple(R.shape)
    if slot not in scratch:
        scratch[slot] = (torch.empty_like(R), torch.empty_like(t), torch.zeros(1, dtype=torch.int64, device=R.device))
    R_n, t_n, word = scratch[slot]
    word.fill_(int(key))
    return ops.pose_jitter(R, t, pose_noise[0], pose_noise[1], word, R_n, t_n, ids=ids)


def imu_noise_key(seed, epoch, minibatch, rank=None):
    """The key of one minibatch's IMU noise and bias draws (--imu_noise_* / --imu_bias_*): pose_noise_key's construction under a salt of
    its own, so a run with both options draws the two independently.  -> the 63 bits mmego_imu_jitter's int64 device word takes."""
    words = (int(seed or 0), int(epoch), int(minibatch)) + (() if rank is None else (int(rank),))
    return _mix64(*words, IMU_NOISE_SALT) & 0x7FFFFFFFFFFFFFFF


def imu_noise_of(cfg):
    """((noise_rot_deg, noise_acc, noise_gyro, bias_rot_deg, bias_acc, bias_gyro), seed) of a run's --imu_noise_* / --imu_bias_* (a
    missing sigma: 0.0; a missing --seed: 0), or None without the flags."""
    given = [getattr(cfg, flag, None) for flag in IMU_NOISE_FLAGS]
    if all(v is None for v in given):
        return None
    return tuple(0.0 if v is None else float(v) for v in given), int(getattr(cfg, "seed", None) or 0)


def imu_noise_line(imu_noise):
    sig, seed = imu_noise
    return ("IMU Noise: white rotation {} deg per axis, accelerometer {}, gyroscope {}; bias rotation {} deg per axis, accelerometer {}, "
            "gyroscope {}; seed {}").format(*sig, seed)


def _jitter_imu(scratch, imu, imu_noise, key, row_ids=None, win_ids=None):
    """An evaluation minibatch's IMU samples [B, T, S, 15] perturbed out of place (buffer and device word kept in ``scratch`` per shape)."""
    imu = imu.contiguous()
    slot = ("imu_noise",) + tuple(imu.shape)
    if slot not in scratch:
        scratch[slot] = (torch.empty_like(imu), torch.zeros(1, dtype=torch.int64, device=imu.device))
    out, word = scratch[slot]
    word.fill_(int(key))
    return ops.imu_jitter(imu, imu_noise[0], word, out, row_ids=row_ids, win_ids=win_ids)


def aligned_summary(m, J):
    """The --metrics full figures from _epoch_eval's columns behind the reference's (m [n_minibatches, 3 J + 3 + nthr + J]): means over
    minibatches of per-minibatch means, lengths in cm.  J = 21: the three joint errors also as means over the upper and the lower joint
    map of the one 21-joint fit."""
    nthr = len(PCK_THRESHOLDS_CM)
    errs = {"root_rel_cm": m[:, :J], "rigid_cm": m[:, J:2 * J], "pa_cm": m[:, 2 * J:3 * J]}
    s = {}
    for name, blk in errs.items():
        s[name] = float(np.mean(blk.mean(axis=1))) * 100
        if J == 21:
            s[name[:-3] + "_upper_cm"] = float(np.mean(blk[:, list(Config.upper_joint_map)].mean(axis=1))) * 100
            s[name[:-3] + "_lower_cm"] = float(np.mean(blk[:, list(Config.lower_joint_map)].mean(axis=1))) * 100
    s["align_rot_deg"] = float(np.mean(m[:, 3 * J]))
    s["align_shift_cm"] = float(np.mean(m[:, 3 * J + 1])) * 100
    s["pa_scale"] = float(np.mean(m[:, 3 * J + 2]))
    s["pck"] = {c: float(np.mean(m[:, 3 * J + 3 + k])) for k, c in enumerate(PCK_THRESHOLDS_CM)}
    acc = m[:, 3 * J + 3 + nthr:]
    s["accel_cm"] = None if np.isnan(acc).any() else float(np.mean(acc.mean(axis=1))) * 100
    s["per_joint_root_rel_cm"] = errs["root_rel_cm"].mean(axis=0) * 100
    s["per_joint_pa_cm"] = errs["pa_cm"].mean(axis=0) * 100
    return s


def _error_summary(sums, n, prefix=""):
    """The reference's five figures from the 43 column sums of mmego_pose_errors over n rows (float64), keys prefixed."""
    m = sums / n
    return {prefix + "all_cm": float(m[:21].mean()) * 100, prefix + "upper_cm": float(m[41]) * 100, prefix + "lower_cm": float(m[42]) * 100,
            prefix + "rot_deg": float(m[21:41].mean()), prefix + "per_joint_cm": m[:21] * 100}


def _accel_over_sequences(dev, up, lo, tgt, spans):
    """Acceleration error over sequences of different lengths: one mmego_pose_accel_errors launch (B = 1, T = its length) per span
    [r0, r1) of the row tensors up [., 45], lo [., 24], tgt [., 63]; spans shorter than 3 rows have no second difference and are left
    out.  -> the mean over ALL interior frames (every sequence weighs by its length - 2) per joint, float64 [21] in metres, or None."""
    spans = [(int(r0), int(r1)) for r0, r1 in spans if r1 - r0 >= 3]
    if not spans:
        return None
    Acc = torch.empty((len(spans), 21), dtype=torch.float32, device=dev)
    for i, (r0, r1) in enumerate(spans):
        n = r1 - r0
        ops.pose_accel_errors(up[r0:r1].view(1, n, 15, 3), lo[r0:r1].view(1, n, 8, 3), tgt[r0:r1].view(1, n, 21, 3), Acc[i:i + 1])
    wt = np.asarray([r1 - r0 - 2 for r0, r1 in spans], dtype=np.float64)
    return (Acc.cpu().numpy().astype(np.float64) * wt[:, None]).sum(axis=0) / wt.sum()


def print_reference(s):
    """The reference's five lines of `--infer` (Demo_test.py), from a summary's all_cm .. per_joint_cm."""
    print("Average Joint Localization Error(cm): {}".format(s["all_cm"]))
    print("Average UpperBody Joint Localization Error(cm): {}".format(s["upper_cm"]))
    print("Average LowerBody Joint Localization Error(cm): {}".format(s["lower_cm"]))
    print("Average Joint Rotation Error(°): {}".format(s["rot_deg"]))
    print("Per Joint Localization Error(cm): {}".format(s["per_joint_cm"]))


def print_aligned(s):
    """The --metrics full lines of `--infer`, from aligned_summary's keys for the 21 joints."""
    for name, parts in (("Root-relative", "root_rel"), ("Rigid-aligned", "rigid"), ("Procrustes-aligned (PA-MPJPE)", "pa")):
        print("{} Joint Error(cm): {} (upper {}, lower {})".format(name, s[parts + "_cm"], s[parts + "_upper_cm"], s[parts + "_lower_cm"]))
    print("Alignment Rotation(°): {}".format(s["align_rot_deg"]))
    print("Alignment Shift(cm): {}".format(s["align_shift_cm"]))
    print("Procrustes Scale: {}".format(s["pa_scale"]))
    for c, v in s["pck"].items():
        print("PCK@{:g}cm: {}".format(c, v))
    print("Acceleration Error(cm/frame^2): {}".format(s["accel_cm"]))
    print("Per Joint Root-relative Error(cm): {}".format(s["per_joint_root_rel_cm"]))
    print("Per Joint Procrustes-aligned Error(cm): {}".format(s["per_joint_pa_cm"]))
