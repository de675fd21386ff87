"""GPU: mmego_pack_frames_noise (csrc/frame_pack.hip) -- mmego_pack_frames with every kept radar return perturbed inside the packer --
against the numpy restatement of its recipe (tests/point_noise_ref.py) bit for bit, on properties that do not lean on the restatement,
on what the launcher refuses, and through data.FrameStore and the Upper trainer under --point_noise / --point_noise_v.  Shapes and frame
lists are those of tests/test_frame_pack_gpu.py, the synthetic recordings those of tests/test_frame_store_gpu.py."""
import numpy as np
import pytest
import torch

import frame_pack_ref as ref
import point_noise_ref as nref
from test_frame_pack_gpu import DEV, R_RTOL, _frames
from test_frame_pack_gpu import _launch as _launch_plain
from test_frame_store_gpu import L, _dataset, _dec

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 63, 64, 65, 127, 128, 129, 174, 300, 0]
FIDX = [9, 0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 3, 9, 5, 0, 7, 7, 10, 8]          # every frame, some twice, out of order; the n = 0 frame too
COPIED = [0, 1, 2, 4, 5]
SPAN = 2.0 * np.sqrt(3.0) * (1.0 + 2.0 ** -22)                               # |z| <= 8388606 C, C within 2^-24 of sqrt(3) 2^-22, one rounding


def _launch(pts, off, fidx, pc_no, max_n, keep_p, seed, sigma_xyz, sigma_v):
    from mmego_amd import ops
    out = torch.full((len(fidx), pc_no, 6), float("nan"), dtype=torch.float32, device=DEV)      # (every row has to be written)
    ops.pack_frames_noise(torch.as_tensor(pts).to(DEV), torch.as_tensor(off).to(DEV), torch.as_tensor(np.asarray(fidx, dtype=np.int64)).to(DEV),
                          out, max_n, keep_p, seed, sigma_xyz, sigma_v)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _within_the_support(noisy, plain, sigma, what):
    """|v' - v| <= 2 sqrt(3) sigma (1 + 2^-22) + ulp: the largest |z|, the product's rounding inside the factor, the sum's rounding below
    one ulp of the larger of the two values."""
    a, b = noisy.astype(np.float64), plain.astype(np.float64)
    slack = SPAN * float(np.float32(sigma)) + np.spacing(np.maximum(np.abs(noisy), np.abs(plain))).astype(np.float64)
    worst = float((np.abs(a - b) / (SPAN * float(np.float32(sigma)))).max()) if a.size and sigma else 0.0
    print("%s: largest |v' - v| is %.4f of 2 sqrt(3) sigma" % (what, worst))
    assert (np.abs(a - b) <= slack).all(), what


def _check_against_ref(pts, off, fidx, pc_no, max_n, keep_p, seed, sigma_xyz, sigma_v):
    got = _launch(pts, off, fidx, pc_no, max_n, keep_p, seed, sigma_xyz, sigma_v)
    want, who = nref.pack_frames_noise(pts, off, fidx, pc_no, max_n, keep_p, seed, sigma_xyz, sigma_v)
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(got[..., COPIED]), _bits(want[..., COPIED])), "x, y, z, velocity, intensity and the zero rows are bit-exact"
    zero = who < 0
    assert np.array_equal(_bits(got[zero]), np.zeros_like(_bits(got[zero])))
    assert np.array_equal(who, ref.pack_frames(pts, off, fidx, pc_no, max_n, keep_p, seed)[1]), "noise moves no return to another slot"
    r = got[..., 3][~zero].astype(np.float64)
    r64 = np.linalg.norm(got[..., 0:3][~zero].astype(np.float64), axis=1)      # of the PERTURBED x, y, z
    rel = np.abs(r - r64) / r64
    print("max relative error of r: %.3g (bound %.3g)" % (rel.max() if rel.size else 0.0, R_RTOL))
    assert (rel <= R_RTOL).all()
    # the intensity is the input's, whichever return sits in the slot
    for q, f in enumerate(fidx):
        src = np.asarray(pts[int(off[f]):int(off[f + 1])], dtype=np.float32).reshape(-1, 5)
        assert np.array_equal(_bits(got[q][~zero[q], 5]), _bits(src[who[q][~zero[q]], 3])), q
    return got, who


@pytest.mark.parametrize("sigmas", [(0.05, 0.0), (0.0, 0.3), (0.05, 0.3)])
@pytest.mark.parametrize("keep_p", [1.0, 0.5])
def test_bit_exact_against_the_restatement(keep_p, sigmas):
    pts, off = _frames(COUNTS)
    got, who = _check_against_ref(pts, off, FIDX, 128, 300, keep_p, 12345, *sigmas)
    assert (who[FIDX.index(10)] < 0).all() and not got[FIDX.index(10)].any()       # n = 0: an all-zero frame
    _check_against_ref(pts, off, FIDX, 128, 174, keep_p, 99, *sigmas)              # max_n below a frame's size
    small, soff = _frames([1, 8, 9], seed=1)
    _check_against_ref(small, soff, [2, 0, 1, 1, 2, 0], 8, 9, keep_p, 7, *sigmas)


@pytest.mark.parametrize("keep_p", [1.0, 0.5])
def test_sigma_zero_is_the_plain_launch(keep_p):
    pts, off = _frames(COUNTS)
    pts[::7, 0] = pts[3::11, 1] = pts[5::13, 2] = pts[2::5, 4] = -0.0
    pts[1] = (-0.0, -0.0, -0.0, 20.0, -0.0)                                        # (r = 0 as well)
    for pc_no, max_n, seed in ((128, 300, 12345), (128, 174, 99)):
        got = _launch(pts, off, FIDX, pc_no, max_n, keep_p, seed, 0.0, 0.0)
        plain = _launch_plain(pts, off, FIDX, pc_no, max_n, keep_p, seed)
        assert (_bits(got[..., 0]) == 0x80000000).any(), "the input's -0.0 reach the output"
        assert np.array_equal(_bits(got), _bits(plain))


def test_properties_without_the_restatement():
    counts = COUNTS[:-1]
    pts, off = _frames(counts, seed=2)
    fidx = list(range(len(counts))) + [5, 8]
    sx, sv = 0.05, 0.3
    for keep_p in (1.0, 0.5):
        plain = _launch_plain(pts, off, fidx, 128, 300, keep_p, 5)
        got = _launch(pts, off, fidx, 128, 300, keep_p, 5, sx, sv)
        assert np.array_equal(_bits(got), _bits(_launch(pts, off, fidx, 128, 300, keep_p, 5, sx, sv)))      # the same seed: the same bytes
        other = _launch(pts, off, fidx, 128, 300, keep_p, 6, sx, sv)
        assert not np.array_equal(_bits(got), _bits(other))
        occ = np.any(plain != 0, axis=2)
        assert np.array_equal(np.any(got != 0, axis=2), occ)                       # the same rows are zero rows
        assert np.array_equal(_bits(got[..., 5]), _bits(plain[..., 5]))            # intensity: never touched
        _within_the_support(got[..., 0:3][occ], plain[..., 0:3][occ], sx, "x, y, z at keep_p %g" % keep_p)
        _within_the_support(got[..., 4][occ], plain[..., 4][occ], sv, "velocity at keep_p %g" % keep_p)
        assert (got[..., COPIED[:4]][occ] != plain[..., COPIED[:4]][occ]).mean() > 0.99      # and hardly a channel keeps its value
        # sigma_xyz = 0: x, y, z and r are the plain launch's bits, the velocity moves
        vel = _launch(pts, off, fidx, 128, 300, keep_p, 5, 0.0, sv)
        assert np.array_equal(_bits(vel[..., [0, 1, 2, 3, 5]]), _bits(plain[..., [0, 1, 2, 3, 5]]))
        assert np.array_equal(_bits(vel[..., 4]), _bits(got[..., 4]))              # (the velocity's draw does not depend on sigma_xyz)
    # a frame listed twice: two independent draws.  Frame 5 has 127 returns and frame 8 has 174: match the copies' rows by their
    # intensity (distinct per return) and compare the noise they carry.
    got = _launch(pts, off, fidx, 128, 300, 1.0, 5, sx, sv)
    for qa, qb, f in ((5, 10, 5), (8, 11, 8)):
        src = pts[off[f]:off[f + 1]]
        assert len(set(src[:, 3].tolist())) == len(src)
        row = {v: j for j, v in enumerate(src[:, 3].tolist())}
        def noise(q):
            rows = got[q][np.any(got[q] != 0, axis=1)]
            j = np.asarray([row[v] for v in rows[:, 5].tolist()])
            return dict(zip(j.tolist(), (rows[:, 0:3] - src[j, 0:3]).tolist()))
        a, b = noise(qa), noise(qb)
        both = sorted(set(a) & set(b))
        assert len(both) >= 64
        da, db = np.asarray([a[j] for j in both]), np.asarray([b[j] for j in both])
        assert (da != db).mean() > 0.99
        assert abs(np.corrcoef(da.ravel(), db.ravel())[0, 1]) < 4.0 / np.sqrt(da.size)      # (4 standard errors of a zero correlation)


def test_launcher_refusals():
    """Non-zero return, nothing launched: the output keeps its fill."""
    from mmego_amd import hip
    pts, off = _frames([5, 7])
    P, O, I = torch.as_tensor(pts).to(DEV), torch.as_tensor(off).to(DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    out = torch.full((2, 128, 6), 3.0, dtype=torch.float32, device=DEV)
    fn = hip.lib().mmego_pack_frames_noise
    st = hip.stream_handle()
    ok = (st, P.data_ptr(), O.data_ptr(), I.data_ptr(), 2, 128, 7, 1.0, 1, 0.05, 0.3, out.data_ptr())
    bad_sigma = (-0.05, float("nan"), float("inf"), float("-inf"))
    for pos, bad in ([(9, s) for s in bad_sigma] + [(10, s) for s in bad_sigma]
                     + [(7, 0.0), (7, 1.5), (7, float("nan")), (5, 0), (5, 1025), (11, None), (1, None), (6, 0), (4, 0)]):
        args = list(ok)
        args[pos] = bad
        assert fn(*args) != 0, (pos, bad)
    args = list(ok)
    args[7], args[9], args[10] = 0.0, 0.0, 0.0                                     # sigma 0, 0 takes the plain kernel: its refusals hold
    assert fn(*args) != 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert fn(*ok) == 0
    torch.cuda.synchronize()
    assert not bool((out == 3.0).any())


# ---- data.FrameStore and the trainer ----------------------------------------------------------------------------------------------------
@pytest.fixture()
def patched(monkeypatch, tmp_path):
    """PosePC reads the synthetic frames; Config as `main.py --train --batch_size 2 --epochs 1` on them would leave it."""
    from mmego_amd import processors
    from mmego_amd.config import Config
    from mmego_amd.data import PosePC
    dec = _dec()
    monkeypatch.setattr(PosePC, "_decode", lambda self: dec)
    for k, v in dict(data_root=str(tmp_path), frame_no=L, batch_size=2, epochs=1, device=DEV, gt_head_pose=True, resume_path=None,
                     finetune_imu=False, finetune_upper=False, finetune_all=False, imu_lr=None, upper_lr=None, imu_dropout=None,
                     clip_grad_norm=None, ema_decay=None, upper_variant="global", metrics="reference", window_jitter=False, point_keep=None,
                     point_noise=None, point_noise_v=None, seed=None, model_upper_path=Config.model_upper_path,
                     model_IMU_path=Config.model_IMU_path).items():
        monkeypatch.setattr(Config, k, v, raising=False)
    monkeypatch.setattr(processors, "_TRAIN_DIR", str(tmp_path / "out"))
    return dec


def test_frame_store_adds_the_noise_to_the_same_packing(patched):
    from mmego_amd.data import FrameStore
    ds = _dataset()
    noisy = FrameStore(ds, DEV, point_keep=0.5, point_noise=0.05, point_noise_v=0.3, seed=3)
    plain = FrameStore(ds, DEV, point_keep=0.5, seed=3)
    idx = np.array([0, 2, 3])
    for minibatch in range(2):
        a, b = noisy.gather(idx), plain.gather(idx)
        if minibatch == 0:
            ptr, first = a["data"].data_ptr(), a["data"].clone()
        assert a["data"].data_ptr() == ptr                                         # the same buffers, a fresh draw
        for k in ("target", "skl", "imu", "R_R0R"):
            assert torch.equal(a[k], b[k]), k
        x, y = a["data"].cpu().numpy().reshape(-1, 128, 6), b["data"].cpu().numpy().reshape(-1, 128, 6)
        occ = np.any(y != 0, axis=2)
        assert np.array_equal(np.any(x != 0, axis=2), occ) and 0 < occ.sum() < ds.frame_npts_[plain.frame_index(idx)].clip(max=128).sum()
        assert np.array_equal(_bits(x[..., 5]), _bits(y[..., 5]))
        _within_the_support(x[..., 0:3][occ], y[..., 0:3][occ], 0.05, "FrameStore x, y, z")
        _within_the_support(x[..., 4][occ], y[..., 4][occ], 0.3, "FrameStore velocity")
        assert (x[..., COPIED[:4]][occ] != y[..., COPIED[:4]][occ]).mean() > 0.99
        r64 = np.linalg.norm(x[..., 0:3][occ].astype(np.float64), axis=1)
        assert (np.abs(x[..., 3][occ] - r64) <= R_RTOL * r64).all()                # r belongs to the perturbed x, y, z
    assert not torch.equal(a["data"], first)
    noisy.begin_epoch(0)
    assert torch.equal(noisy.gather(idx)["data"], first)                           # a function of (seed, epoch, minibatch)
    with pytest.raises(ValueError, match="belong to gather"):
        noisy.gather_field_into("data", idx, torch.empty_like(first))
    # noise alone keeps every return: the slots of point_keep = 1 under the same seed
    alone, keep1 = FrameStore(ds, DEV, point_noise=0.05, seed=3), FrameStore(ds, DEV, point_keep=1.0, seed=3)
    assert alone.point_keep is None and alone.pts is not None
    x = alone.gather(np.arange(4))["data"].cpu().numpy().reshape(-1, 128, 6)
    y = keep1.gather(np.arange(4))["data"].cpu().numpy().reshape(-1, 128, 6)
    occ = np.any(y != 0, axis=2)
    assert np.array_equal(np.any(x != 0, axis=2), occ)
    assert np.array_equal(occ.sum(axis=1), ds.frame_npts_[alone.frame_index(np.arange(4))].clip(max=128))
    assert np.array_equal(_bits(x[..., 4:6]), _bits(y[..., 4:6])) and (x[..., 0:3][occ] != y[..., 0:3][occ]).mean() > 0.99
    with pytest.raises(ValueError, match="belong to gather"):
        alone.gather_field_into("data", np.arange(4), torch.empty(4, L, 128, 6, device=DEV))


def _train_upper(noise, noise_v):
    """One epoch of the Upper trainer, built as main.py --seed 1 builds it -> (the loss log, the weights)."""
    from mmego_amd import processors
    from mmego_amd.config import Config
    Config.point_noise, Config.point_noise_v, Config.seed = noise, noise_v, 1
    torch.manual_seed(1)
    np.random.seed(1)
    log = []
    tr = processors.UpperTrainer()
    once = tr.train_once
    tr.train_once = lambda: (log.append(once()), log[-1])[1]
    tr.train_upper()
    assert isinstance(tr._train_dev, processors.FrameStore) is (noise is not None or noise_v is not None)
    for f in (getattr(tr, "lossfile", None), getattr(tr, "evalfile", None)):
        if f is not None:
            f.close()
    flat = np.asarray([v for e in log for part in (e if isinstance(e, tuple) else (e,)) for v in np.ravel(part)], dtype=np.float64)
    assert len(log) == 1 and np.isfinite(flat).all()
    torch.cuda.synchronize()
    return flat, {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}


def test_upper_trainer_end_to_end(patched, capsys):
    la, a = _train_upper(0.02, 0.1)
    said = capsys.readouterr().out
    assert "return noise sigma xyz 0.02, velocity 0.1" in said
    lb, b = _train_upper(0.02, 0.1)
    capsys.readouterr()
    lc, c = _train_upper(None, None)
    assert "frame store" not in capsys.readouterr().out                            # without the flags: DeviceArrays, and no word of it
    assert np.array_equal(la, lb) and a.keys() == b.keys() == c.keys()
    assert all(torch.equal(a[k], b[k]) for k in a), "the same flags and seed: the same weights, bit for bit"
    assert all(bool(torch.isfinite(v).all()) for v in a.values() if v.is_floating_point())
    assert any(not torch.equal(a[k], c[k]) for k in a), "without the flags: other weights"
