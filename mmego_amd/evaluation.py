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


# ---- the error breakdown (--breakdown): by action, by recording, percentiles -------------------------------------------------------
BREAKDOWN_BINS = (0.05, 4096)                                            # --breakdown: (bin_cm, nbins), 0.05 cm bins up to 204.75 cm
BREAKDOWN_QUANTILES = (50, 90, 95, 99)
PCK_AUC_UPTO_CM = 15.0


def check_breakdown(breakdown):
    """breakdown = (bin_cm, nbins) of evaluate_full / dense_infer, or None.  -> (bin_cm, nbins) as a float and an int.  Refused
    (ValueError): a bin_cm that is not finite and > 0, nbins outside [2, 4096] (the last bin is the overflow bin), a 100 / bin_cm -- the
    bins per metre the kernel multiplies by -- that is not a float32 exactly."""
    if breakdown is None:
        return None
    if not (isinstance(breakdown, (tuple, list)) and len(breakdown) == 2):
        raise ValueError("breakdown: (bin_cm, nbins), got %r" % (breakdown,))
    bin_cm, nbins = breakdown
    if isinstance(bin_cm, bool) or not isinstance(bin_cm, (int, float, np.integer, np.floating)) or not 0.0 < bin_cm < float("inf"):
        raise ValueError("breakdown: bin_cm is a finite number of centimetres > 0, got %r" % (bin_cm,))
    if isinstance(nbins, bool) or not isinstance(nbins, (int, np.integer)) or not 2 <= nbins <= ops.HIST_MAX_BINS:
        raise ValueError("breakdown: nbins is an integer in [2, %d], got %r" % (ops.HIST_MAX_BINS, nbins))
    inv = 100.0 / float(bin_cm)
    if not ops.is_float32(inv):
        raise ValueError("breakdown: 100 / bin_cm = %r bins per metre is not a float32 exactly, so the device's bins would not be "
                         "bin_cm wide; take a bin_cm such as 0.05, 0.1, 0.125, 0.5" % inv)
    return float(bin_cm), int(nbins)


def hist_quantile(hist, bin_width, q):
    """The q-quantile (0 < q <= 1) of a histogram whose LAST bin is the overflow bin, bins ``bin_width`` wide from 0.  -> (value,
    clipped).  n = hist.sum(); the first bin b with cum[b] >= q n holds it, and the value is interpolated linearly inside that bin,
    (b + (q n - cum[b - 1]) / hist[b]) * bin_width -- within one bin width of the order statistic x_(ceil(q n)).  Where b is the overflow
    bin nothing bounds the value from above: its lower edge is returned and clipped is True.  An empty histogram: (None, False)."""
    if not 0.0 < q <= 1.0:
        raise ValueError("hist_quantile: q lies in (0, 1], got %r" % (q,))
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    n = int(hist.sum())
    if n == 0:
        return None, False
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, q * n, side="left"))             # the first bin with cum[b] >= q n
    if b >= len(hist) - 1:
        return (len(hist) - 1) * float(bin_width), True
    below = int(cum[b - 1]) if b else 0
    return (b + (q * n - below) / float(hist[b])) * float(bin_width), False


def pck_auc_edges(nbins, bin_width, upto_cm=PCK_AUC_UPTO_CM):
    """K: the bin edges k * bin_width, k = 1 .. K, that pck_auc averages over -- those <= upto_cm (to a relative 1e-9: 300 * 0.05 is
    15.000000000000002 in float64) that are edges of regular bins, k <= nbins - 1."""
    return int(min(np.floor(float(upto_cm) / float(bin_width) * (1.0 + 1e-9)), nbins - 1))


def pck_auc(hist, bin_width, upto_cm=PCK_AUC_UPTO_CM):
    """The area under the PCK curve from 0 to upto_cm, as a fraction of the full area: the mean over the bin edges k * bin_width <=
    upto_cm, k >= 1, of PCK@(k * bin_width) = cum[k - 1] / n (a value on an edge belongs to the bin above it, so PCK here is 'error <
    threshold').  None for an empty histogram or a bin wider than upto_cm."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    n, K = int(hist.sum()), pck_auc_edges(len(hist), bin_width, upto_cm)
    if n == 0 or K < 1:
        return None
    return float(np.cumsum(hist)[:K].astype(np.float64).sum() / (float(n) * K))


def dataset_groups(dataset):
    """(win_rec, rec_action, rec_snippet) of a loader's split: the recording of every ITEM of ``dataset`` (PosePC's win_rec_ cut as its
    items are) and the two per-recording arrays.  ValueError for a split that does not carry them (an ArraySplit)."""
    if any(getattr(dataset, k, None) is None for k in ("win_rec_", "rec_action_", "rec_snippet_")):
        raise ValueError("breakdown: the split has no win_rec_ / rec_action_ / rec_snippet_ (a data.PosePC has); there is nothing to group by")
    n, cut = len(dataset.win_rec_), dataset.split_cut
    sl = slice(0, n) if dataset.vis else (slice(0, cut) if dataset.train else slice(cut, n))
    win_rec = np.asarray(dataset.win_rec_[sl], dtype=np.int64)
    if len(win_rec) != len(dataset):
        raise ValueError("breakdown: win_rec_ names %d windows, the split has %d" % (len(win_rec), len(dataset)))
    return win_rec, np.asarray(dataset.rec_action_, dtype=np.int64), np.asarray(dataset.rec_snippet_, dtype=np.int64)


class Breakdown:
    """One pass's breakdown: the group ids of its rows, the launches over its finished tables, and the summary from what came down.
    row_rec [rows]: every row's recording, -1 for a row that does not count (an uncovered frame); rec_action, rec_snippet: per recording.
    The float results live behind the pass's own figure log in ONE flat buffer (floats()), so they come down in the pass's one read; the
    histograms are one int32 buffer, one further read."""

    def __init__(self, breakdown, row_rec, rec_action, rec_snippet, full, device):
        self.bin_cm, self.nbins = check_breakdown(breakdown)
        self.full, self.device = bool(full), device
        self.rec_action, self.rec_snippet = np.asarray(rec_action, dtype=np.int64), np.asarray(rec_snippet, dtype=np.int64)
        self.actions = np.unique(self.rec_action)                                   # ascending directory numbers
        self.n_act, self.n_rec = len(self.actions), len(self.rec_action)
        row_rec = np.asarray(row_rec, dtype=np.int64)
        self.rows = len(row_rec)
        if self.n_rec < 1 or self.n_rec > ops.GROUPS_MAX_G or not 1 <= self.rows < ops.GROUPS_MAX_ROWS:
            raise ValueError("breakdown: %d rows of %d recordings do not fit the grouped sums" % (self.rows, self.n_rec))
        if row_rec.max() >= self.n_rec:
            raise ValueError("breakdown: a row names recording %d of %d" % (row_rec.max(), self.n_rec))
        counted = row_rec >= 0
        act_of_rec = np.searchsorted(self.actions, self.rec_action)
        ids = np.stack([np.where(counted, act_of_rec[np.maximum(row_rec, 0)], -1), np.where(counted, row_rec, -1), np.where(counted, 0, -1)])
        self._ids_host = np.ascontiguousarray(ids.astype(np.int32))                 # [3, rows]: by action, by recording, all counted rows
        self.every_row = bool(counted.all())

    # the flat float buffer's fields, in order: name -> shape
    def _fields(self):
        f = [("act_sum", (self.n_act, 43)), ("act_n", (self.n_act,)), ("rec_sum", (self.n_rec, 43)), ("rec_n", (self.n_rec,))]
        if self.full:
            f += [("act_pa", (self.n_act, 21)), ("act_root_rel", (self.n_act, 21))]
        return f

    def floats(self):
        return sum(int(np.prod(shape)) for _, shape in self._fields())

    def _views(self, flat):
        v, o = {}, 0
        for name, shape in self._fields():
            n = int(np.prod(shape))
            v[name], o = flat[o:o + n].reshape(shape), o + n
        return v

    def launch(self, E, A, flat):
        """The launches over the pass's finished tables E [rows, >= 43] (mmego_pose_errors' columns) and, under "full", A (the columns
        of mmego_pose_errors_aligned for 21 joints): grouped sums into ``flat`` (floats() floats behind the pass's log), the three
        histograms of the 21 joint errors -- all counted rows pooled, pooled by action, per joint -- into one int32 buffer, returned."""
        ids = torch.as_tensor(self._ids_host).to(self.device)
        v = self._views(flat)
        ops.colsum_groups(E[:, :43], ids[0], self.n_act, v["act_sum"], v["act_n"])
        ops.colsum_groups(E[:, :43], ids[1], self.n_rec, v["rec_sum"], v["rec_n"])
        if self.full:
            ops.colsum_groups(A[:, 42:63], ids[0], self.n_act, v["act_pa"])
            ops.colsum_groups(A[:, :21], ids[0], self.n_act, v["act_root_rel"])
        nb, nh = self.nbins, 1 + self.n_act + 21
        H = torch.empty(nh * (nb + 1), dtype=torch.int32, device=self.device)       # [nh, nbins] histograms, then [nh] dropped counts
        hist, lost = H[:nh * nb].view(nh, nb), H[nh * nb:]
        J, w = E[:, :21], 100.0 / self.bin_cm                                    # (bins per metre: check_breakdown held it to a float32)
        ops.hist_groups(J, None if self.every_row else ids[2], 1, w, nb, hist[:1], lost[:1])
        ops.hist_groups(J, ids[0], self.n_act, w, nb, hist[1:1 + self.n_act], lost[1:1 + self.n_act])
        ops.hist_groups(J, None if self.every_row else ids[2], 1, w, nb, hist[1 + self.n_act:].view(1, 21, nb), lost[1 + self.n_act:].view(1, 21),
                        pool=False)
        return H

    def summary(self, flat, H):
        """breakdown_summary's keys from the downloaded float fields and histogram buffer (host arrays)."""
        v = self._views(np.asarray(flat, dtype=np.float64))
        nb, nh = self.nbins, 1 + self.n_act + 21
        H = np.asarray(H, dtype=np.int64)
        hist, lost = H[:nh * nb].reshape(nh, nb), H[nh * nb:]
        return breakdown_summary(self, v, hist, lost)


def breakdown_summary(bd, v, hist, lost):
    """The summary keys of a breakdown from the grouped sums ``v`` (Breakdown's fields, float64), the histograms hist [1 + n_act + 21,
    nbins] (all, by action, per joint) and their dropped counts.  Every group figure is a PLAIN MEAN over the group's frames."""
    w = bd.bin_cm
    quant = lambda h, q: hist_quantile(h, w, q / 100.0)

    def means(sums, n):
        ok = n > 0
        m = sums / np.where(ok, n, 1.0)[:, None]
        return m, ok
    some = lambda x, ok: [float(a) if k else None for a, k in zip(x, ok)]
    m, ok = means(v["act_sum"], v["act_n"])
    rec_ok = v["rec_n"] > 0
    by_action = dict(action=[int(a) for a in bd.actions], frames=[int(n) for n in v["act_n"]],
                     recordings=[int(np.count_nonzero(rec_ok & (bd.rec_action == a))) for a in bd.actions],
                     all_cm=some(m[:, :21].mean(axis=1) * 100, ok), upper_cm=some(m[:, 41] * 100, ok), lower_cm=some(m[:, 42] * 100, ok),
                     rot_deg=some(m[:, 21:41].mean(axis=1), ok),
                     p50_cm=[quant(hist[1 + i], 50)[0] for i in range(bd.n_act)], p90_cm=[quant(hist[1 + i], 90)[0] for i in range(bd.n_act)])
    if bd.full:
        by_action.update(pa_cm=some(means(v["act_pa"], v["act_n"])[0].mean(axis=1) * 100, ok),
                         root_rel_cm=some(means(v["act_root_rel"], v["act_n"])[0].mean(axis=1) * 100, ok))
    mr, _ = means(v["rec_sum"], v["rec_n"])
    by_recording = dict(recording=list(range(bd.n_rec)), action=[int(a) for a in bd.rec_action], snippet=[int(j) for j in bd.rec_snippet],
                        frames=[int(n) for n in v["rec_n"]], all_cm=some(mr[:, :21].mean(axis=1) * 100, rec_ok))
    qs = {q: quant(hist[0], q) for q in BREAKDOWN_QUANTILES}
    return dict(by_action=by_action, by_recording=by_recording, percentiles_cm={q: qs[q][0] for q in qs},
                percentile_clipped=any(c for _, c in qs.values()), beyond=int(hist[0, -1]), joint_errors=int(hist[0].sum()),
                dropped=int(lost[0]), per_joint_median_cm=np.asarray([np.nan if quant(h, 50)[0] is None else quant(h, 50)[0]
                                                                      for h in hist[1 + bd.n_act:]]),
                pck_auc=pck_auc(hist[0], w), error_hist=hist[0].copy(), breakdown=(bd.bin_cm, bd.nbins))


def print_breakdown(s):
    """The --breakdown lines, behind everything else a pass prints."""
    p, (bin_cm, nbins), a = s["percentiles_cm"], s["breakdown"], s["by_action"]
    print("Joint Error Percentiles(cm): p50 {} p90 {} p95 {} p99 {} (bins of {} cm; {} of {} joint errors beyond {} cm)".format(
        p[50], p[90], p[95], p[99], bin_cm, s["beyond"], s["joint_errors"], (nbins - 1) * bin_cm))
    print("PCK AUC(0-{:g}cm): {}".format(PCK_AUC_UPTO_CM, s["pck_auc"]))
    print("Per Joint Median Error(cm): {}".format(s["per_joint_median_cm"]))
    for i, act in enumerate(a["action"]):
        line = "Action {} ({} frames, {} recordings): all {} upper {} lower {} rotation(°) {} p50 {} p90 {}".format(
            act, a["frames"][i], a["recordings"][i], a["all_cm"][i], a["upper_cm"][i], a["lower_cm"][i], a["rot_deg"][i], a["p50_cm"][i],
            a["p90_cm"][i])
        if "pa_cm" in a:
            line += " pa {} root-relative {}".format(a["pa_cm"][i], a["root_rel_cm"][i])
        print(line)
    r = s["by_recording"]
    worst = sorted((i for i in range(len(r["recording"])) if r["all_cm"][i] is not None), key=lambda i: -r["all_cm"][i])[:5]
    print("Worst Recordings(cm): " + "; ".join("action {} snippet {}: {} ({} frames)".format(r["action"][i], r["snippet"][i], r["all_cm"][i],
                                                                                           r["frames"][i]) for i in worst))
