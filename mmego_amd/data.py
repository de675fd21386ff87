"""Sample_data loader: per-frame .mat files -> fixed-size windows of radar points, skeletons, IMU and head pose.

Counterpart of the reference's Util/Universal_Util/Dataset_sample.py:12-277 (class PosePC) -- same constructor,
same per-item tuples, same array attributes.  The numpy global RNG is consumed in the same order as the
reference (one choice() per frame for the slot layout, plus the reference's unused second draw), so
``np.random.seed(k)`` before construction reproduces the reference's padded point clouds bit for bit
(checked in tests/test_data_cpu.py against tests/golden/real16.npz).
"""
import glob
import hashlib
import os
import re

import numpy as np
import scipy.io as scio

from .config import Config

CACHE_VERSION = 1

R_RI = np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0]])
R_TTB = np.array([[0, -1, 0], [-1, 0, 0], [0, 0, -1]])
R_CTW = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])


def _numeric_key(path):
    return [int(tok) for tok in re.findall(r"\d+", os.path.basename(path))]


def list_snippets(root):
    """[(action_index, snippet_index, [frame files...])] in the reference's traversal order."""
    out = []
    actions = sorted(os.listdir(root), key=lambda name: int(name))
    for a, action in enumerate(actions):
        adir = os.path.join(root, action)
        for j, snip in enumerate(sorted(os.listdir(adir))):
            sdir = os.path.join(adir, snip)
            if not os.path.isdir(sdir):
                continue
            frames = sorted(glob.glob(os.path.join(sdir, "*.mat")), key=_numeric_key)
            if frames and not (a == 0 and j == 0):           # the reference skips the very first snippet
                out.append((a, j, frames))
    return out


def pack_points(raw, pc_no):
    """(n,5) x,y,z,intensity,velocity -> (pc_no,6) x,y,z,range,velocity,intensity, zero-padded at random slots
    or randomly subsampled (Dataset_sample.py:203-224)."""
    n = raw.shape[0]
    pts = np.zeros((n, 6), dtype=np.float32)
    pts[:, 0:3] = raw[:, :3]
    pts[:, 3] = np.linalg.norm(raw[:, 0:3], axis=1)
    pts[:, 4] = raw[:, 4]
    pts[:, 5] = raw[:, 3]
    if n < pc_no:
        slots = np.random.choice(pc_no, size=n, replace=False)
        np.random.choice(n, size=pc_no - n, replace=True)      # drawn and discarded by the reference; keeps RNG in step
        frame = np.zeros((pc_no, 6), dtype=np.float32)
        frame[slots] = pts
        return frame
    return pts[np.random.choice(n, size=pc_no, replace=False)]


def imu_to_radar_frame(imu, orientation_ref):
    """Rotate the 20x(9+3+3) IMU samples into the radar frame and fix signs/gravity (Dataset_sample.py:183-192).
    Mutates and returns ``imu``."""
    R_ni = np.stack([imu[:, :3], imu[:, 3:6], imu[:, 6:9]], axis=2)
    rot = R_RI @ (orientation_ref.T @ R_ni) @ R_RI.T
    imu[:, :3], imu[:, 3:6], imu[:, 6:9] = rot[:, 0, :], rot[:, 1, :], rot[:, 2, :]
    imu[:, 11] = imu[:, 11] + 9.8
    imu[:, 10:12] = -1 * imu[:, 10:12]
    imu[:, 13:] = -1 * imu[:, 13:]
    return imu


class PosePC:
    """Dataset of non-overlapping ``frame_no``-frame windows (taken from the tail of each recording)."""

    def __init__(self, train=True, vis=False, batch_length=None, root=None, keep_frames=False):
        """keep_frames (for FrameStore): the per-frame packed clouds, which are packed anyway, stay in ``frame_packed_`` instead of being
        dropped after the windows are cut.  The other per-frame views (``frame_pts_`` ... ``win_start_``) are the decoded arrays
        themselves and are always there; nothing else about the object depends on the keyword."""
        self.vis, self.train = vis, train
        self._keep_frames = bool(keep_frames)
        self.pc_no = Config.pc_no
        self.frame_no = batch_length if batch_length is not None else Config.frame_no
        self.joint_selection = Config.kinect_joint_selection
        self.skeleton = Config.skeleton_all.tolist()
        self.root = root or Config.data_root
        (self.data_ti_, self.data_key_, self.imu_, self.skl_, self.ground_, self.foot_contact_, self.R_R0R_,
         self.t_R0R_, self.R_RtW_) = self._read()
        n = len(self.data_ti_)
        if not vis:
            order = np.arange(n)
            np.random.RandomState(Config.dataset_random_seed).shuffle(order)    # same permutation as shuffling each array
            for name in ("data_ti_", "data_key_", "skl_", "ground_", "foot_contact_", "imu_", "R_R0R_", "t_R0R_", "win_start_", "win_rec_"):
                setattr(self, name, getattr(self, name)[order])
        cut = int(n * 0.8)
        self.split_cut = n if vis else cut              # windows [0, split_cut) of the arrays train, the rest test
        sl = slice(0, n) if vis else (slice(0, cut) if train else slice(cut, n))
        self._items = [getattr(self, k)[sl] for k in ("data_ti_", "data_key_", "skl_", "imu_", "ground_",
                                                      "foot_contact_", "R_R0R_", "t_R0R_")]
        if vis:
            self._items.append(self.R_RtW_)

    def __len__(self):
        return len(self._items[0])

    def __getitem__(self, i):
        return tuple(a[i] for a in self._items)

    # -----------------------------------------------------------------------------------------
    def _decode(self):
        """Everything that comes out of the .mat files and does NOT depend on numpy's RNG: per snippet, per non-empty
        frame the raw points and the derived small arrays.  This is the slow part of the reference's start-up (one
        scipy.loadmat per frame, 19 208 files = 14 s, done twice: train and test set) and it is deterministic, so it is
        kept in a packed binary cache: one .npz per (file list, sizes, mtimes)."""
        snippets = list_snippets(self.root)
        cache = _cache_path(self.root, snippets, self.joint_selection, self.skeleton)
        if cache and os.path.exists(cache):
            try:
                z = np.load(cache, allow_pickle=False)
                return {k: z[k] for k in z.files}
            except (OSError, ValueError, KeyError):
                pass
        fr = {k: [] for k in ("pts", "npts", "key", "imu", "ground", "foot", "R", "t", "RtW")}
        snip_len = []
        ref = None          # (R_btc, imu orientation, bone vectors) of the first frame ever read
        for _, _, files in snippets:
            count = 0
            for path in files:
                m = scio.loadmat(path)
                raw = np.asarray(m["pc_xyziv_ti2"][:, 0:5].tolist())
                if len(raw) == 0:
                    continue
                joints = np.asarray([m["pc_xyz_key_2"][:, 0:3][i] for i in self.joint_selection])
                imu = m["imu_save_l"]
                if ref is None:
                    bones = [joints[p] - joints[c] for p, c in self.skeleton]
                    ref = (m["R_btc"], np.asarray(m["orientation_imu_img"]), bones)
                R_btc = m["R_btc"]
                fr["R"].append(R_TTB @ ref[0] @ R_btc.T @ R_TTB.T)
                fr["RtW"].append(R_TTB @ R_btc @ R_CTW)
                fr["imu"].append(imu_to_radar_frame(imu, ref[1]))
                fc = m["foot_contact"]
                fr["foot"].append([[0, 1] if fc[0, 0] else [1, 0], [0, 1] if fc[0, 1] else [1, 0]])
                ground = m["abcd_ground_2"]
                fr["ground"].append(-1 * ground if ground[0, 0] > 0 else ground)
                fr["pts"].append(raw)
                fr["npts"].append(len(raw))
                fr["key"].append(joints)
                fr["t"].append(m["t_R0R"])
                count += 1
            snip_len.append(count)
        dec = {"pts": np.concatenate(fr["pts"], 0) if fr["pts"] else np.zeros((0, 5)), "npts": np.asarray(fr["npts"], dtype=np.int64),
               "snip_len": np.asarray(snip_len, dtype=np.int64),
               "bones": np.asarray(ref[2]) if ref is not None else np.zeros((0, 3))}
        for k in ("key", "imu", "ground", "foot", "R", "t", "RtW"):
            dec[k] = np.asarray(fr[k])
        if cache:
            try:
                os.makedirs(os.path.dirname(cache), exist_ok=True)
                tmp = cache + ".tmp%d.npz" % os.getpid()
                np.savez(tmp, **dec)
                os.replace(tmp, cache)
            except OSError:
                pass                                    # read-only location: work without a cache
        return dec

    def _read(self):
        if not os.path.isdir(self.root):
            raise FileNotFoundError("Sample_data not found at %s (set MMEGO_DATA_ROOT or Config.data_root)" % self.root)
        dec = self._decode()
        win = {k: [] for k in ("ti", "key", "imu", "skl", "ground", "foot", "R", "t", "RtW")}
        bones = [b for b in dec["bones"]]
        packed, starts, win_rec = [], [], []             # every frame's packed cloud; every window's first frame (global number) and recording
        f0 = 0                                           # first frame of the snippet in the packed arrays
        p0 = 0                                           # first point of that frame in dec["pts"]
        for rec_no, count in enumerate(dec["snip_len"]):
            rec = {k: [] for k in ("ti", "key", "imu", "ground", "foot", "R", "t", "RtW")}
            for f in range(f0, f0 + int(count)):
                n = int(dec["npts"][f])
                rec["ti"].append(pack_points(dec["pts"][p0:p0 + n], self.pc_no))     # consumes numpy's RNG like the reference
                if self._keep_frames:
                    packed.append(rec["ti"][-1])
                p0 += n
                for k in ("key", "imu", "ground", "foot", "R", "t", "RtW"):
                    rec[k].append(dec[k][f])
            f0 += int(count)
            L = self.frame_no
            while len(rec["ti"]) >= L:
                starts.append(f0 - int(count) + len(rec["ti"]) - L)
                win_rec.append(rec_no)
                for k in rec:
                    win[k].append(rec[k][-L:])
                    rec[k] = rec[k][:-L]
                win["skl"].append(bones)
        # the per-frame views (FrameStore): the decoded arrays as they are, the recording number of every frame, the packed clouds of
        # ALL frames (the head of a recording that fills no window included), and every window's first frame in data_ti_'s order
        nf = len(dec["npts"])
        self.frame_pts_, self.frame_npts_ = dec["pts"], np.asarray(dec["npts"], dtype=np.int64)
        self.frame_key_, self.frame_imu_, self.frame_R_ = dec["key"], dec["imu"], dec["R"]
        # the floor of every frame, in the frame of its own joints (after _decode's sign rule), and the recorded contact flags: column 0
        # belongs to joint 15, column 1 to joint 19 (dense inference's floor figures read them; nothing else does)
        self.frame_ground_ = np.asarray(dec["ground"], dtype=np.float32).reshape(nf, 4)
        self.frame_contact_ = np.asarray(dec["foot"]).reshape(nf, 2, 2)[:, :, 1].astype(np.uint8)
        self.frame_rec_ = np.repeat(np.arange(len(dec["snip_len"]), dtype=np.int64), np.asarray(dec["snip_len"], dtype=np.int64))
        self.frame_bones_ = np.asarray(dec["bones"])
        self.frame_packed_ = (np.asarray(packed, dtype=np.float32).reshape(nf, self.pc_no, 6) if self._keep_frames else None)
        self.win_start_ = np.asarray(starts, dtype=np.int64)
        # where every recording comes from (recording r is list_snippets(root)[r], as in frame_rec_): the integer its action directory is
        # named by and the snippet's position among that directory's entries (None where the decoded frames are not this tree's); and
        # every window's recording, in data_ti_'s order
        try:
            snippets = list_snippets(self.root)
            names = sorted(os.listdir(self.root), key=lambda name: int(name))
        except (OSError, ValueError):                    # (frames decoded elsewhere, served under a root that is no Sample_data tree)
            snippets, names = [], []
        known = len(snippets) == len(dec["snip_len"]) > 0
        self.rec_action_ = np.asarray([int(names[a]) for a, _, _ in snippets], dtype=np.int64) if known else None
        self.rec_snippet_ = np.asarray([j for _, j, _ in snippets], dtype=np.int64) if known else None
        self.win_rec_ = np.asarray(win_rec, dtype=np.int64)
        print("data load end")
        return tuple(np.asarray(win[k]) for k in ("ti", "key", "imu", "skl", "ground", "foot", "R", "t", "RtW"))


def _cache_path(root, snippets, joint_selection, skeleton):
    """Cache file of the decoded frames of ``root``: keyed by every frame file's path, size and mtime (and by the joint
    selection).  MMEGO_CACHE_DIR overrides the location (default ~/.cache/mmego_amd); MMEGO_CACHE_DIR=off disables it."""
    base = os.environ.get("MMEGO_CACHE_DIR", os.path.join(os.path.expanduser("~"), ".cache", "mmego_amd"))
    if base == "off":
        return None
    h = hashlib.sha256()
    h.update(("v%d|%s|%s|%s" % (CACHE_VERSION, os.path.abspath(root), list(joint_selection), skeleton)).encode())
    for _, _, files in snippets:
        for path in files:
            st = os.stat(path)
            h.update(("%s|%d|%d" % (path, st.st_size, st.st_mtime_ns)).encode())
    return os.path.join(base, "frames_%s.npz" % h.hexdigest()[:24])


class DeviceArrays:
    """The training arrays of a PosePC resident in HBM as fp32 (uploaded once: 835 x 20 x 128 x 6 floats = 51 MB for
    Sample_data), with minibatches gathered ON the device by index (mmego_gather_rows).  Replaces the reference's
    per-batch numpy stacking + float64->float32 `torch.tensor(...)` + host->device copies (Train_Upper.py:140-150);
    the values are the same (the one rounding to fp32 happens at upload instead of per batch)."""

    FIELDS = (("data", 0), ("target", 1), ("skl", 2), ("imu", 3), ("R_R0R", 6))

    def __init__(self, dataset, device):
        import torch
        self.n = len(dataset)
        self.device = device
        self.src, self.shape = {}, {}
        for name, i in self.FIELDS:
            a = np.ascontiguousarray(dataset._items[i])
            self.shape[name] = tuple(a.shape[1:])
            self.src[name] = torch.as_tensor(a.reshape(self.n, -1), dtype=torch.float32).to(device)
        self._out = {}

    @staticmethod
    def of(dataset, device):
        """The device copy of ``dataset``, uploaded once per dataset OBJECT and shared by everybody who evaluates or trains on
        it.  The copy hangs on the dataset itself (not in a table keyed by id(): an id can be reused after garbage collection), is
        dropped with it, and is rebuilt when the dataset's length or its arrays' identity changed (a split mutated in place)."""
        stamp = (str(device), len(dataset)) + tuple(id(dataset._items[i]) for _, i in DeviceArrays.FIELDS)
        ent = dataset.__dict__.get("_device_arrays")
        if ent is None or ent[0] != stamp:
            ent = dataset.__dict__["_device_arrays"] = (stamp, DeviceArrays(dataset, device))
        return ent[1]

    def gather(self, index):
        """index: int array of item numbers -> dict of device tensors [len(index), ...] (buffers reused per batch size)."""
        import torch
        from . import ops
        idx = torch.as_tensor(np.ascontiguousarray(index), dtype=torch.int64).to(self.device)
        B = idx.numel()
        out = {}
        for name, _ in self.FIELDS:
            key = (name, B)
            dst = self._out.get(key)
            if dst is None:
                dst = torch.empty((B, self.src[name].shape[1]), dtype=torch.float32, device=self.device)
                self._out[key] = dst
            ops.gather_rows(self.src[name], idx, dst)
            out[name] = dst.view((B,) + self.shape[name])
        return out


def _gather_field_into(self, name, index, out):
    """One field of the items `index` into a caller-owned buffer `out` [len(index), ...] (the prefetch of the NEXT minibatch's
    IMU samples for train_step.PipelinedStages, which must not disturb the current minibatch's buffers)."""
    import torch
    from . import ops
    idx = torch.as_tensor(np.ascontiguousarray(index), dtype=torch.int64).to(self.device)
    ops.gather_rows(self.src[name], idx, out.view(idx.numel(), -1))
    return out


DeviceArrays.gather_field_into = _gather_field_into


def _mix64(*words):
    """One 64-bit word from a tuple of integers (splitmix64 steps): the seeds FrameStore derives from (seed, epoch, ...)."""
    M = 0xFFFFFFFFFFFFFFFF
    s = 0x6A09E667F3BCC908
    for w in words:
        s = (s + (int(w) & M) + 0x9E3779B97F4A7C15) & M
        s = ((s ^ (s >> 30)) * 0xBF58476D1CE4E5B9) & M
        s = ((s ^ (s >> 27)) * 0x94D049BB133111EB) & M
        s ^= s >> 31
    return s


class FrameStore:
    """The training split of a PosePC resident in HBM FRAME-major (about 110 MB for Sample_data: per frame the IMU samples, the
    skeleton, the head rotation and the host-packed cloud, plus the raw radar returns with CSR offsets), with minibatches of windows
    assembled ON the device from any window start -- the device-side counterpart of DeviceArrays for the two options that DeviceArrays'
    finished windows cannot serve:

      jitter       begin_epoch(epoch) moves every training window to a start drawn uniformly from the VALID starts within
                   +-(frame_no - 1) frames of its own: starts whose frame_no frames lie in one recording and touch no frame of a
                   test window (frames that belong to no window are fair game).  A window without such freedom keeps its start.
      point_keep   every gather packs the raw returns of its frames afresh on the device (mmego_pack_frames): each return kept with
                   probability point_keep, the survivors at random slots (or a random ordered subsample of them), as pack_points does
                   once per load on the host.  1.0 only re-draws the packing.
      point_noise, point_noise_v   (finite floats > 0) the same per-gather packing with every kept return perturbed inside the packer
                   (mmego_pack_frames_noise): x, y, z by point_noise z, the Doppler velocity by point_noise_v z, z of unit variance and
                   support +-2 sqrt(3); r follows the perturbed x, y, z.  Without point_keep every return is kept (keep_p = 1: the
                   packing is re-drawn, as under point_keep = 1).

    All off: the reference's windows and the loader's packing -- gather() returns what DeviceArrays(dataset).gather() returns.
    The start draws come from a RandomState of their own seeded by (seed, epoch), the packing seeds from (seed, epoch, minibatch
    number): neither touches the RNG of the minibatch order, every data-parallel rank draws the same starts, and a run resumed
    at an epoch continues the same sequence.  ``index`` of gather / gather_field_into holds training-window numbers, as for
    DeviceArrays; the buffers are static per minibatch size and `data` is a fresh copy every call (the nets transform it in place)."""

    UNUSED, TRAIN, TEST = 0, 1, 2
    FIELDS = DeviceArrays.FIELDS

    def __init__(self, dataset, device, jitter=False, point_keep=None, seed=0, point_noise=None, point_noise_v=None):
        import torch
        from . import ops
        if getattr(dataset, "frame_packed_", None) is None:
            raise ValueError("FrameStore needs the per-frame clouds: build the PosePC with keep_frames=True")
        if dataset.vis or not dataset.train:
            raise ValueError("FrameStore serves the training split of a PosePC(train=True)")
        if point_keep is not None and not 0.0 < float(point_keep) <= 1.0:
            raise ValueError("point_keep is a probability in (0, 1], got %r" % (point_keep,))
        for name, v in (("point_noise", point_noise), ("point_noise_v", point_noise_v)):
            if v is not None and not 0.0 < float(v) < float("inf"):          # (false for NaN as well)
                raise ValueError("%s is a standard deviation, finite and > 0 (None: no noise), got %r" % (name, v))
        self.device, self.n = device, len(dataset)
        self.jitter, self.point_keep, self.seed = bool(jitter), None if point_keep is None else float(point_keep), int(seed)
        self.point_noise = None if point_noise is None else float(point_noise)
        self.point_noise_v = None if point_noise_v is None else float(point_noise_v)
        self.noisy = self.point_noise is not None or self.point_noise_v is not None
        self.repack = self.point_keep is not None or self.noisy          # `data` is packed per gather from the raw returns
        self.L, self.pc_no = L, pc_no = int(dataset.frame_no), int(dataset.pc_no)
        self.F = F = len(dataset.frame_npts_)
        # who owns a frame: the one PosePC knows both sides of the split
        cut = dataset.split_cut
        self.ref_starts = np.asarray(dataset.win_start_[:cut], dtype=np.int64)
        self.owner = np.zeros(F, dtype=np.int8)
        span = np.arange(L)
        self.owner[(self.ref_starts[:, None] + span).ravel()] = self.TRAIN
        self.owner[(np.asarray(dataset.win_start_[cut:], dtype=np.int64)[:, None] + span).ravel()] = self.TEST
        # valid starts: frame_no frames of one recording, none of them a test frame
        rec = np.asarray(dataset.frame_rec_)
        ntest = np.concatenate([[0], np.cumsum(self.owner == self.TEST)])
        s = np.arange(max(F - L + 1, 0))
        self._valid = (rec[s] == rec[s + L - 1]) & (ntest[s + L] == ntest[s]) if len(s) else np.zeros(0, dtype=bool)
        # per training window: the valid starts within +-(L-1) of its own, as one CSR list
        cand = []
        for s0 in self.ref_starts:
            lo, hi = max(int(s0) - (L - 1), 0), min(int(s0) + (L - 1), F - L)
            cand.append(lo + np.nonzero(self._valid[lo:hi + 1])[0])
        self._cand_len = np.asarray([len(c) for c in cand], dtype=np.int64)
        if (self._cand_len < 1).any():
            raise ValueError("a training window's own start is not valid: the dataset's windows and split do not belong together")
        self._cand_off = np.concatenate([[0], np.cumsum(self._cand_len)])[:-1]
        self._cand = np.concatenate(cand) if cand else np.zeros(0, dtype=np.int64)
        self.n_movable = int((self._cand_len > 1).sum())
        # the split in HBM, frame-major
        f32 = lambda a, rows: torch.as_tensor(np.ascontiguousarray(a).reshape(rows, -1), dtype=torch.float32).to(device)
        self.shape = {name: tuple(np.shape(dataset._items[i])[1:]) for name, i in self.FIELDS}
        self.src = {"imu": f32(dataset.frame_imu_, F), "target": f32(dataset.frame_key_, F), "R_R0R": f32(dataset.frame_R_, F),
                    "data": f32(dataset.frame_packed_, F), "skl": f32(dataset.frame_bones_, 1)}
        self.width = {name: self.src[name].shape[1] for name in self.src}
        npts = np.asarray(dataset.frame_npts_, dtype=np.int64)
        self.max_n = int(npts.max()) if F else 1
        self.pts = self.off = None
        if self.repack:
            if pc_no > ops.PACK_FRAMES_MAX_PC_NO or self.max_n > ops.pack_frames_max_n(pc_no):
                raise ValueError("a frame of %d points at pc_no = %d is beyond what mmego_pack_frames' 64 KB of LDS hold (at most %d points)"
                                 % (self.max_n, pc_no, ops.pack_frames_max_n(pc_no)))
            pts = np.asarray(dataset.frame_pts_, dtype=np.float32).reshape(-1, 5)
            self.pts = torch.as_tensor(pts if len(pts) else np.zeros((1, 5), np.float32)).to(device)
            self.off = torch.as_tensor(np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)).to(device)
        self._out, self._zero_idx = {}, {}
        self.begin_epoch(0)

    def valid_starts(self):
        """Every s for which frames s .. s+frame_no-1 lie in one recording and none is a test frame."""
        return np.nonzero(self._valid)[0]

    def begin_epoch(self, epoch):
        """The epoch's window starts (jitter: one draw per training window from RandomState(seed, epoch)) and minibatch counter."""
        self.epoch, self._minibatch = int(epoch), 0
        if not self.jitter:
            self.starts = self.ref_starts
            return self.starts
        s = _mix64(self.seed, self.epoch, 0x4A495454)
        rs = np.random.RandomState([s & 0xFFFFFFFF, s >> 32])
        k = np.minimum((rs.random_sample(self.n) * self._cand_len).astype(np.int64), self._cand_len - 1)
        self.starts = self._cand[self._cand_off + k]
        return self.starts

    def frame_index(self, index):
        """Host: the frame numbers [len(index) * frame_no] of the windows ``index`` at this epoch's starts."""
        fi = (self.starts[np.asarray(index, dtype=np.int64)][:, None] + np.arange(self.L)).ravel()
        if len(fi) and (fi.min() < 0 or fi.max() >= self.F):
            raise IndexError("window start outside the frame arrays")
        return np.ascontiguousarray(fi)

    def _upload(self, index):
        import torch
        return torch.as_tensor(self.frame_index(index)).to(self.device), len(index)

    def _field(self, name, fidx, B, dst, pack_seed):
        import torch
        from . import ops
        if name == "skl":                                   # one bone set for the whole recording campaign: row 0, B times
            z = self._zero_idx.get(B)
            if z is None:
                z = self._zero_idx[B] = torch.zeros(B, dtype=torch.int64, device=self.device)
            return ops.gather_rows(self.src["skl"], z, dst.view(B, -1))
        if name == "data" and self.repack:
            keep = 1.0 if self.point_keep is None else self.point_keep
            if self.noisy:
                return ops.pack_frames_noise(self.pts, self.off, fidx, dst.view(B * self.L, self.pc_no, 6), self.max_n, keep, pack_seed,
                                             self.point_noise or 0.0, self.point_noise_v or 0.0)
            return ops.pack_frames(self.pts, self.off, fidx, dst.view(B * self.L, self.pc_no, 6), self.max_n, keep, pack_seed)
        return ops.gather_rows(self.src[name], fidx, dst.view(B * self.L, self.width[name]))

    def gather(self, index):
        """index: int array of training-window numbers -> dict of device tensors [len(index), ...] (buffers reused per batch size)."""
        import torch
        fidx, B = self._upload(index)
        pack_seed = _mix64(self.seed, self.epoch, self._minibatch, 0x5041434B)
        self._minibatch += 1
        out = {}
        for name, _ in self.FIELDS:
            key = (name, B)
            dst = self._out.get(key)
            if dst is None:
                dst = torch.empty((B,) + self.shape[name], dtype=torch.float32, device=self.device)
                self._out[key] = dst
            self._field(name, fidx, B, dst, pack_seed)
            out[name] = dst
        return out

    def gather_field_into(self, name, index, out):
        """One field of the windows `index`, at this epoch's starts, into a caller-owned buffer (DeviceArrays.gather_field_into)."""
        if name == "data" and self.repack:
            raise ValueError("the re-drawn clouds belong to gather(): their seed is its minibatch counter")
        fidx, B = self._upload(index)
        self._field(name, fidx, B, out, 0)
        return out


BLENDS = ("mean", "triangle")


class DensePlan:
    """Sliding-window inference, host side: overlapping ``T``-frame windows at a stride ``S`` in [1, T] over recordings of the given
    lengths (frame-major: recording i owns the global frames [a_i, b_i)), and for every frame the list of window rows that cover it.

      windows   a recording shorter than T has none (its frames stay uncovered); otherwise the starts are b - T - k S, k = 0, 1, ...
                while >= a, united with a: tail-anchored like PosePC's grid, so at S = T they are PosePC's windows plus one head window
                per recording whose length is no multiple of T.  Windows are numbered recording by recording, ascending start.
      starts    [W] first global frame of every window;  recording [W] its recording
      row_frame [W T] int64: the global frame of window row w T + p
      cover     of frame f, as CSR: cov_off [F + 1] int64, cov_row [nnz] int32 (rows w T + p, ascending w within a frame), cov_w [nnz]
                fp32 (blend "mean": 1; "triangle": min(p + 1, T - p), the window's middle counts most); covered [F] the counts.
    Every frame of a recording of at least T frames is covered, at most ceil(T / S) + 1 times.
    lookahead=L, an integer in [0, T - 1] (None, the default: every array as above): the CAUSAL cover of a device that may answer for
    frame f no later than L frames after it.  The windows do not move (starts, recording, row_frame, W); window row r of window
    w = r // T, whose last frame is e = starts[w] + T - 1, stays in the cover of frame f only where e <= f + L, and cov_off, cov_row,
    cov_w, covered and max_cover are those of the rows that stay, the weights those of ``blend``.  L = T - 1 is the cover above, byte
    for byte.  The first T - 1 - L frames of every recording of at least T frames are covered by nothing -- the WARM-UP, a device has
    no full window yet -- and ``warmup`` counts them (0 without lookahead); every later frame is covered if and only if S <= L + 1, so
    a larger stride is refused."""

    def __init__(self, lengths, T, stride, blend="mean", lookahead=None):
        T, S = int(T), int(stride)
        if T < 1 or not 1 <= S <= T:
            raise ValueError("dense windows: the stride has to lie in [1, %d] (a larger one leaves frames between windows uncovered), got %r"
                             % (T, stride))
        if blend not in BLENDS:
            raise ValueError("blend: %r is not one of %s" % (blend, ", ".join(BLENDS)))
        if lookahead is not None:
            if isinstance(lookahead, bool) or not isinstance(lookahead, (int, np.integer)) or not 0 <= lookahead <= T - 1:
                raise ValueError("dense windows: lookahead is an integer number of frames in [0, %d], got %r" % (T - 1, lookahead))
            if S > lookahead + 1:
                raise ValueError("dense windows: under lookahead %d a frame is served by a window that ends at most %d frames after it, "
                                 "so a stride above %d leaves frames between windows uncovered, got %d"
                                 % (lookahead, lookahead, lookahead + 1, S))
            lookahead = int(lookahead)
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.T, self.stride, self.blend, self.lookahead = T, S, blend, lookahead
        self.F = F = int(lengths.sum())
        self.rec_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        starts, recs = [], []
        for i, (a, b) in enumerate(zip(self.rec_off[:-1], self.rec_off[1:])):
            if b - a < T:
                continue
            s = np.arange(b - T, a - 1, -S, dtype=np.int64)[::-1]
            if s[0] != a:
                s = np.concatenate([[a], s])
            starts.append(s)
            recs.append(np.full(len(s), i, dtype=np.int64))
        self.starts = np.concatenate(starts).astype(np.int64) if starts else np.zeros(0, np.int64)
        self.recording = np.concatenate(recs) if recs else np.zeros(0, np.int64)
        self.W = W = len(self.starts)
        self.row_frame = np.ascontiguousarray((self.starts[:, None] + np.arange(T, dtype=np.int64)).ravel())
        if W * T >= 2 ** 31:
            raise ValueError("dense windows: %d window rows do not fit the cover's int32 row numbers" % (W * T))
        order = np.argsort(self.row_frame, kind="stable")           # rows by frame; within a frame in row order = ascending window
        if lookahead is not None:                                   # the rows whose window had ended by their frame + L: position p >= T - 1 - L
            order = order[order % T >= T - 1 - lookahead]
        self.cov_row = np.ascontiguousarray(order.astype(np.int32))
        self.covered = np.bincount(self.row_frame[order], minlength=F).astype(np.int64)
        self.cov_off = np.concatenate([[0], np.cumsum(self.covered)]).astype(np.int64)
        p = self.cov_row % T
        self.cov_w = (np.ones(len(p), np.float32) if blend == "mean" else np.minimum(p + 1, T - p).astype(np.float32))
        self.max_cover = int(self.covered.max()) if F else 0
        self.frame_rec = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
        self.frame_in_recording = np.arange(F, dtype=np.int64) - self.rec_off[:-1][self.frame_rec]
        self.warmup = 0 if lookahead is None else int((lengths >= T).sum()) * (T - 1 - lookahead)


class DenseWindows(DensePlan):
    """The DensePlan of a PosePC(train=False, vis=True, keep_frames=True, batch_length=T) with the recordings resident in HBM frame-major
    (the five fields of FrameStore.src, uploaded once) and windows assembled on the device from the plan's starts.  Every frame keeps the
    one packed cloud the loader drew for it, whichever window it is served in: a run is a function of its inputs alone."""

    FIELDS = DeviceArrays.FIELDS

    def __init__(self, dataset, device, stride, blend="mean", lookahead=None):
        import torch
        if getattr(dataset, "frame_packed_", None) is None:
            raise ValueError("DenseWindows needs the per-frame clouds: build the PosePC with keep_frames=True")
        if not dataset.vis:
            raise ValueError("DenseWindows serves whole recordings: build the PosePC with train=False, vis=True")
        F = len(dataset.frame_npts_)
        nrec = int(dataset.frame_rec_.max()) + 1 if F else 0
        super().__init__(np.bincount(np.asarray(dataset.frame_rec_, dtype=np.int64), minlength=nrec), dataset.frame_no, stride, blend,
                         lookahead=lookahead)
        self.device, self.pc_no = device, int(dataset.pc_no)
        f32 = lambda a, rows: torch.as_tensor(np.ascontiguousarray(a).reshape(rows, -1), dtype=torch.float32).to(device)
        T = self.T
        self.shape = {"data": (T, self.pc_no, 6), "target": (T,) + tuple(np.shape(dataset.frame_key_)[1:]),
                      "skl": tuple(np.shape(dataset.frame_bones_)), "imu": (T,) + tuple(np.shape(dataset.frame_imu_)[1:]),
                      "R_R0R": (T,) + tuple(np.shape(dataset.frame_R_)[1:])}
        self.src = {"imu": f32(dataset.frame_imu_, F), "target": f32(dataset.frame_key_, F), "R_R0R": f32(dataset.frame_R_, F),
                    "data": f32(dataset.frame_packed_, F), "skl": f32(dataset.frame_bones_, 1)}
        self.width = {name: self.src[name].shape[1] for name in self.src}
        self.bone_set = np.asarray(dataset.frame_bones_, dtype=np.float32).reshape(-1, 3).copy()     # host: src["skl"] row 0 as [20, 3]
        self._out, self._zero_idx = {}, {}
        self._dataset, self._floor, self._ground = dataset, None, None
        # every recording's action (the integer its directory is named by), for the error breakdown; None from a loader without it
        act = getattr(dataset, "rec_action_", None)
        self.rec_action = None if act is None else np.asarray(act, dtype=np.int64)
        self.rec_snippet = None if act is None else np.asarray(dataset.rec_snippet_, dtype=np.int64)

    def floor(self):
        """-> (ground [F, 4], contact [F, 2]): every frame's floor plane and contact flags as fp32 device tensors, uploaded on the first
        call (dense inference's floor figures; a pass without them never calls this and uploads nothing)."""
        import torch
        if self._floor is None:
            ds = self._dataset
            if getattr(ds, "frame_ground_", None) is None or getattr(ds, "frame_contact_", None) is None:
                raise ValueError("DenseWindows.floor needs the loader's frame_ground_ and frame_contact_")
            ground, contact = np.asarray(ds.frame_ground_), np.asarray(ds.frame_contact_)
            if ground.shape != (self.F, 4) or contact.shape != (self.F, 2):
                raise ValueError("DenseWindows.floor: frame_ground_ %s and frame_contact_ %s do not belong to %d frames"
                                 % (ground.shape, contact.shape, self.F))
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
            self._floor = (up(ground), up(contact))
        return self._floor

    def ground(self):
        """-> ground [F, 4]: every frame's floor plane alone, an fp32 device tensor (floor()'s where that was uploaded): dense inference's
        pictures need the plane and no contact flags.  ValueError where the loader has no frame_ground_ of F rows."""
        import torch
        if self._floor is not None:
            return self._floor[0]
        if self._ground is None:
            ground = getattr(self._dataset, "frame_ground_", None)
            if ground is None or np.asarray(ground).shape != (self.F, 4):
                raise ValueError("DenseWindows.ground needs the loader's frame_ground_ [%d, 4], got %s"
                                 % (self.F, None if ground is None else np.asarray(ground).shape))
            self._ground = torch.as_tensor(np.ascontiguousarray(ground, dtype=np.float32)).to(self.device)
        return self._ground

    def frame_index(self, index):
        """Host: the frame numbers [len(index) * T] of the windows ``index``."""
        index = np.asarray(index, dtype=np.int64)
        if len(index) and (index.min() < 0 or index.max() >= self.W):
            raise IndexError("window number outside the plan's %d windows" % self.W)
        return np.ascontiguousarray((self.starts[index][:, None] + np.arange(self.T)).ravel())

    def gather(self, index):
        """index: int array of window numbers -> dict of device tensors [len(index), T, ...] like DeviceArrays.gather (buffers reused per
        batch size; `data` is a fresh copy every call: the nets transform it in place)."""
        import torch
        from . import ops
        fidx, B = torch.as_tensor(self.frame_index(index)).to(self.device), len(index)
        out = {}
        for name, _ in self.FIELDS:
            dst = self._out.get((name, B))
            if dst is None:
                dst = self._out[(name, B)] = torch.empty((B,) + self.shape[name], dtype=torch.float32, device=self.device)
            if name == "skl":                                   # one bone set for the whole recording campaign: row 0, B times
                z = self._zero_idx.get(B)
                if z is None:
                    z = self._zero_idx[B] = torch.zeros(B, dtype=torch.int64, device=self.device)
                ops.gather_rows(self.src["skl"], z, dst.view(B, -1))
            else:
                ops.gather_rows(self.src[name], fidx, dst.view(B * self.T, self.width[name]))
            out[name] = dst
        return out


class ArraySplit:
    """A data split given as arrays (what PosePC exposes to the trainers: `_items` in the reference loader's tuple order
    data, target, skl, imu, ground, foot_contact, R_R0R, t_R0R -- Dataset_sample.py:264-277).  For callers that hold windows
    already (tests, fixtures)."""

    def __init__(self, data, target, skl, imu, R_R0R):
        n = len(data)
        z = np.zeros((n, 1), dtype=np.float32)
        self._items = [np.asarray(data), np.asarray(target), np.asarray(skl), np.asarray(imu), z, z, np.asarray(R_R0R), z]

    def __len__(self):
        return len(self._items[0])

    def __getitem__(self, i):
        return tuple(a[i] for a in self._items)


def batch_indices(n, batch_size, shuffle, rng=None):
    """The index sets `batches` iterates over (same RNG consumption), for on-device gathering."""
    order = (rng or np.random).permutation(n) if shuffle else np.arange(n)
    for s in range(0, n, batch_size):
        yield order[s:s + batch_size]


def batches(dataset, batch_size, shuffle, rng=None):
    """Minibatch iterator (the reference uses torch DataLoader(num_workers=0, drop_last=False)): yields tuples of
    stacked numpy arrays."""
    n = len(dataset)
    order = (rng or np.random).permutation(n) if shuffle else np.arange(n)
    for s in range(0, n, batch_size):
        idx = order[s:s + batch_size]
        yield tuple(a[idx] for a in dataset._items)
