"""GPU: data.FrameStore -- the training split frame-major in HBM, minibatches of windows assembled on the device from any window
start, clouds re-drawn per minibatch by mmego_pack_frames -- against DeviceArrays (options off), against the host re-assembly at
the drawn starts (jitter), and through the three trainers with --window_jitter / --point_keep.  The set: three recordings of 9, 13
and 5 frames, windows of 4 frames (6 windows: 4 train, 2 test), 128 slots, frames of 2 to 150 returns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L = 4
SNIPS = (9, 13, 5)


def _dec():
    rng = np.random.default_rng(42)
    F = sum(SNIPS)
    npts = rng.integers(2, 100, F).astype(np.int64)
    npts[[3, 11, 20]] = (150, 128, 129)
    q = np.linalg.qr(rng.normal(size=(F, 3, 3)))[0]
    skel = rng.normal(0, 0.4, (21, 3)) + np.array([0.8, 0.0, 0.2])
    imu = np.concatenate([np.tile(q.reshape(F, 1, 9), (1, 20, 1)), rng.normal(size=(F, 20, 6))], axis=2)
    pts = np.concatenate([rng.normal([0.8, 0.0, 0.2], 0.4, (int(npts.sum()), 3)), rng.uniform(10, 46, (int(npts.sum()), 1)),
                          rng.normal(0, 0.4, (int(npts.sum()), 1))], axis=1)
    return {"pts": pts, "npts": npts, "snip_len": np.asarray(SNIPS, dtype=np.int64), "bones": 0.2 * rng.normal(size=(20, 3)),
            "key": skel + rng.normal(0, 0.01, (F, 21, 3)), "imu": imu, "ground": np.zeros((F, 1, 4), np.float32),
            "foot": np.zeros((F, 2, 2), np.int64), "R": q, "t": rng.normal(size=(F, 1, 3)), "RtW": q}


@pytest.fixture()
def patched(monkeypatch, tmp_path):
    """PosePC reads the synthetic frames; Config as `main.py --train --batch_size 2 --epochs 2` on them would leave it."""
    from mmego_amd import processors
    from mmego_amd.config import Config
    from mmego_amd.data import PosePC
    dec = _dec()
    monkeypatch.setattr(PosePC, "_decode", lambda self: dec)
    for k, v in dict(data_root=str(tmp_path), frame_no=L, batch_size=2, epochs=2, device=DEV, gt_head_pose=True, resume_path=None,
                     finetune_imu=False, finetune_upper=False, finetune_all=False, imu_lr=None, upper_lr=None, imu_dropout=None,
                     clip_grad_norm=None, upper_variant="global", metrics="reference", window_jitter=False, point_keep=None, seed=None,
                     model_upper_path=Config.model_upper_path, model_IMU_path=Config.model_IMU_path).items():
        monkeypatch.setattr(Config, k, v, raising=False)
    monkeypatch.setattr(processors, "_TRAIN_DIR", str(tmp_path / "out"))
    return dec


def _dataset(seed=0):
    from mmego_amd.data import PosePC
    np.random.seed(seed)
    return PosePC(train=True, batch_length=L, keep_frames=True)


FIELDS = ("data", "target", "skl", "imu", "R_R0R")


def test_options_off_equals_device_arrays(patched):
    from mmego_amd.data import DeviceArrays, FrameStore
    ds = _dataset()
    assert len(ds) == 4 and len(ds.win_start_) == 6
    fs, da = FrameStore(ds, DEV), DeviceArrays(ds, DEV)
    for idx in (np.array([2, 0, 3]), np.array([1]), np.arange(4), np.array([3, 3])):
        a, b = fs.gather(idx), da.gather(idx)
        for name in FIELDS:
            assert a[name].shape == b[name].shape and torch.equal(a[name], b[name]), name


def _host(ds, starts, idx):
    fi = starts[idx][:, None] + np.arange(L)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
    return {"data": f32(ds.frame_packed_[fi]), "target": f32(ds.frame_key_[fi]), "imu": f32(ds.frame_imu_[fi]), "R_R0R": f32(ds.frame_R_[fi]),
            "skl": f32(np.broadcast_to(ds.frame_bones_, (len(idx), 20, 3)))}


def test_jitter_gathers_the_drawn_windows(patched):
    from mmego_amd.data import FrameStore
    ds = _dataset()
    fs = FrameStore(ds, DEV, jitter=True, seed=3)
    assert fs.n_movable >= 2 and len(fs.valid_starts()) > 6
    moved = 0
    for epoch in range(3):
        starts = fs.begin_epoch(epoch).copy()
        moved += int((starts != fs.ref_starts).sum())
        for idx in (np.array([2, 0, 3]), np.array([1, 1])):
            got, want = fs.gather(idx), _host(ds, starts, idx)
            for name in FIELDS:
                assert torch.equal(got[name].cpu(), want[name]), (epoch, name)
            nxt = torch.full((len(idx), L, 20, 15), float("nan"), device=DEV)
            assert fs.gather_field_into("imu", idx, nxt) is nxt and torch.equal(nxt, got["imu"])
    assert moved > 0


def test_point_keep_redraws_into_the_same_buffers(patched):
    import frame_pack_ref as ref
    from mmego_amd import nets
    from mmego_amd.data import FrameStore, _mix64
    ds = _dataset()
    fs = FrameStore(ds, DEV, jitter=True, point_keep=0.8, seed=3)
    idx = np.array([0, 2])
    a = fs.gather(idx)
    first = {k: v.clone() for k, v in a.items()}
    ptr = a["data"].data_ptr()
    # the first minibatch of epoch 0 is the restatement's packing under the seed of (seed, epoch, minibatch)
    off = np.concatenate([[0], np.cumsum(ds.frame_npts_)])
    want, who = ref.pack_frames(np.asarray(ds.frame_pts_, np.float32), off, fs.frame_index(idx), 128, fs.max_n, 0.8, _mix64(3, 0, 0, 0x5041434B))
    got = first["data"].cpu().numpy().reshape(-1, 128, 6)
    assert np.array_equal(got[..., [0, 1, 2, 4, 5]], want[..., [0, 1, 2, 4, 5]])
    assert (who >= 0).sum() < ds.frame_npts_[fs.frame_index(idx)].clip(max=128).sum()          # (some returns were dropped)
    # a net's in-place transform of `data` (quirk Q1) reaches no memory of the store: the next gather is a fresh draw from clean sources
    a["data"].mul_(0.0).add_(7.0)
    src = {k: v.clone() for k, v in fs.src.items()}
    pts = fs.pts.clone()
    b = fs.gather(idx)
    assert b["data"].data_ptr() == ptr and all(b[k].data_ptr() == a[k].data_ptr() for k in FIELDS)
    assert not torch.equal(b["data"], first["data"]) and not bool((b["data"] == 7.0).any())
    for k in ("target", "skl", "imu", "R_R0R"):
        assert torch.equal(b[k], first[k]), k
    assert torch.equal(fs.pts, pts) and all(torch.equal(fs.src[k], src[k]) for k in src)
    # the same (seed, epoch, minibatch) again: the same clouds
    fs.begin_epoch(0)
    assert torch.equal(fs.gather(idx)["data"], first["data"]) and torch.equal(fs.gather(idx)["data"], b["data"])
    # point_keep = 1 only re-draws the packing: every frame keeps min(n, 128) returns
    fs1 = FrameStore(ds, DEV, point_keep=1.0, seed=3)
    d = fs1.gather(np.arange(4))["data"].cpu().numpy().reshape(-1, 128, 6)
    assert np.array_equal(np.any(d != 0, axis=2).sum(axis=1), ds.frame_npts_[fs1.frame_index(np.arange(4))].clip(max=128))
    assert not np.array_equal(d, ds.data_ti_[:4].reshape(-1, 128, 6))


def _run(kind, seed, jitter=True, keep=0.8):
    """One trainer, built as main.py builds it, for Config.epochs epochs -> what every training pass returned (the loss log)."""
    from mmego_amd import processors
    from mmego_amd.config import Config
    Config.window_jitter, Config.point_keep, Config.seed = jitter, keep, seed
    torch.manual_seed(0)                     # (the nets and the loader's packing: the same in every run -- only the store's seed changes)
    np.random.seed(0)
    log = []
    if kind == "imu":
        tr = processors.ImuTrainer()
        once = tr.train_imu_once
        tr.train_imu_once = lambda: (log.append(once()), log[-1])[1]
        tr.train_imu()
    else:
        tr = processors.UpperTrainer() if kind == "upper" else processors.LowerTrainer()
        once = tr.train_once
        tr.train_once = lambda: (log.append(once()), log[-1])[1]
        tr.train_upper() if kind == "upper" else tr.train_lower()
    assert isinstance(tr._train_dev, processors.FrameStore) and tr._train_dev.epoch == Config.epochs - 1
    for f in (getattr(tr, "lossfile", None), getattr(tr, "evalfile", None)):
        if f is not None:
            f.close()
    flat = np.asarray([v for e in log for part in (e if isinstance(e, tuple) else (e,)) for v in np.ravel(part)], dtype=np.float64)
    assert len(log) == Config.epochs and np.isfinite(flat).all()
    return flat


def test_upper_trainer_end_to_end(patched):
    a, b, c = _run("upper", 3), _run("upper", 3), _run("upper", 4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_lower_trainer_end_to_end(patched, tmp_path):
    from mmego_amd import nets
    from mmego_amd.config import Config
    torch.manual_seed(1)
    Config.model_upper_path = str(tmp_path / "upper.pth")
    torch.save(nets.UpperNet().state_dict(), Config.model_upper_path)
    a, b, c = _run("lower", 3), _run("lower", 3), _run("lower", 4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_imu_trainer_with_window_jitter(patched):
    from mmego_amd.config import Config
    Config.epochs = 1
    a, b, c = _run("imu", 3, keep=None), _run("imu", 3, keep=None), _run("imu", 4, keep=None)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_pipelined_imu_engine_sees_the_jittered_starts(patched, tmp_path, monkeypatch):
    """The frozen IMU_Net's forward runs one minibatch ahead on gather_field_into("imu", ...): under jitter it gives the loss log of
    MMEGO_PIPELINE_IMU=0, where the IMU samples come from gather() itself."""
    from mmego_amd import nets
    from mmego_amd.config import Config
    torch.manual_seed(1)
    Config.gt_head_pose, Config.model_IMU_path = False, str(tmp_path / "imu.pth")
    torch.save(nets.IMUNet(15, 9, 512, 2, True, 0.1).state_dict(), Config.model_IMU_path)
    monkeypatch.delenv("MMEGO_PIPELINE_IMU", raising=False)
    a = _run("upper", 3, keep=None)
    monkeypatch.setenv("MMEGO_PIPELINE_IMU", "0")
    b = _run("upper", 3, keep=None)
    assert np.array_equal(a, b)
