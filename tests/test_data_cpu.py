"""CPU: the Sample_data loader reproduces the reference loader's arrays (tests/golden/real16.npz), from the stored frames and
layout of tests/golden/g11_loader.npz (made by tests/golden/make_loader_fixture.py from the reference's data directory)."""
import os

import numpy as np
import scipy.io as scio

from conftest import golden

MAT_KEYS = ("pc_xyziv_ti2", "pc_xyz_key_2", "imu_save_l", "R_btc", "orientation_imu_img", "t_R0R", "abcd_ground_2", "foot_contact")


def _mat_tree(root, g):
    """The first snippet in use back as .mat files, behind the (empty) snippet the loader skips: the stored frames as they
    were, every other frame with its point count and zeros (it reaches window 0 only through numpy's RNG)."""
    action, skipped, snip = [str(s) for s in g["mat.dirs"]]
    os.makedirs(os.path.join(root, action, skipped))
    d = os.path.join(root, action, snip)
    os.makedirs(d)
    npts, full = g["mat.npts"].astype(np.int64), [int(i) for i in g["mat.full"]]
    p0 = np.concatenate([[0], np.cumsum(npts[full])])
    per = {k: g["mat." + k] for k in MAT_KEYS}
    for i, name in enumerate(g["mat.names"]):
        if i in full:
            j = full.index(i)
            m = {"pc_xyziv_ti2": per["pc_xyziv_ti2"][p0[j]:p0[j + 1]]}
            for k in MAT_KEYS[1:]:
                r = len(per[k]) // len(full)
                m[k] = per[k][j * r:(j + 1) * r]
        else:
            m = {"pc_xyziv_ti2": np.zeros((npts[i], 5), np.float32), "pc_xyz_key_2": np.zeros((32, 3)), "imu_save_l": np.zeros((20, 15)),
                 "R_btc": np.eye(3), "orientation_imu_img": np.eye(3), "t_R0R": np.zeros((1, 3)),
                 "abcd_ground_2": np.zeros((1, 4), np.float32), "foot_contact": np.zeros((1, 2), np.uint8)}
        scio.savemat(os.path.join(d, str(name)), m)


def _decoded(g, real, L=20, pc_no=128):
    """The loader's decoded frames of the whole set, rebuilt from the stored layout and real16.npz: the frames of the 16 pinned
    windows carry the reference's values, every other frame zeros of the right size.  The points of a pinned frame are put back
    in their file order by replaying the reference's draws from seed 0 (Dataset_sample.py's pack step: per frame, slots for n < 128
    points plus a discarded second draw, else a subsample of 128) -- a loader that draws differently does not get real16's clouds
    back; points the subsample drops stay zero."""
    npts = g["dec.npts"].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(npts)])
    where = {}                                           # frame -> (row of real16, position in the window)
    windows, f0 = 0, 0
    sel = [int(w) for w in real["sel"]]
    for count in g["dec.snip_len"].astype(np.int64):
        end = f0 + int(count)
        while end - f0 >= L:
            if windows in sel:
                for i in range(L):
                    where[end - L + i] = (sel.index(windows), i)
            windows += 1
            end -= L
        f0 += int(count)
    assert windows == 835 and len(where) == 16 * L
    dec = {"pts": np.zeros((int(starts[-1]), 5)), "npts": npts, "snip_len": g["dec.snip_len"].astype(np.int64), "bones": g["dec.bones"]}
    for k, shape, dt in (("key", (21, 3), np.float64), ("imu", (20, 15), np.float64), ("ground", (1, 4), np.float32),
                         ("foot", (2, 2), np.int64), ("R", (3, 3), np.float64), ("t", (1, 3), np.float64), ("RtW", (3, 3), np.float64)):
        dec[k] = np.zeros((len(npts),) + shape, dtype=dt)
    rng = np.random.RandomState(0)
    for f, n in enumerate(npts):
        if n < pc_no:
            draw = rng.choice(pc_no, size=n, replace=False)
            rng.choice(n, size=pc_no - n, replace=True)
        else:
            draw = rng.choice(n, size=pc_no, replace=False)
        if f not in where:
            continue
        r, i = where[f]
        packed = real["x"][r, i][:, [0, 1, 2, 5, 4]].astype(np.float64)      # (x, y, z, range, velocity, intensity) -> file columns
        raw = dec["pts"][starts[f]:starts[f + 1]]
        if n < pc_no:
            raw[:] = packed[draw]
        else:
            raw[draw] = packed
        dec["key"][f], dec["imu"][f], dec["R"][f] = real["target"][r, i], real["imu"][r, i], real["R"][r, i]
    return dec


def test_loader_matches_reference_arrays(tmp_path, monkeypatch):
    from mmego_amd.config import Config
    from mmego_amd.data import PosePC, batches
    real, g = golden("real16.npz"), golden("g11_loader.npz")
    sel = real["sel"]
    # the whole loader (.mat decoding, rotations, windows, point packing) on the first snippet in use: its last 20 frames are
    # window 0 of the set, and numpy's RNG has been consumed by the same frames before them
    root = str(tmp_path / "Sample_data")
    _mat_tree(root, g)
    assert sel[0] == 0
    np.random.seed(0)                                    # the seed make_golden.py used before the reference loader
    ds = PosePC(train=False, vis=True, batch_length=20, root=root)
    assert len(ds) == len(g["mat.names"]) // 20
    assert np.array_equal(ds.data_ti_[0], real["x"][0]), "padded point clouds must be bit-identical under the same seed"
    assert np.array_equal(ds.data_key_[0].astype(np.float32), real["target"][0])
    assert np.array_equal(ds.skl_[0].astype(np.float32), real["skl"][0])
    assert np.array_equal(ds.R_R0R_[0].astype(np.float32), real["R"][0])
    assert np.array_equal(ds.imu_[0].astype(np.float32), real["imu"][0])
    # the whole set from its decoded layout: windows, the RNG over all 19 114 frames, the 16 pinned windows, the split
    dec = _decoded(g, real)
    monkeypatch.setattr(PosePC, "_decode", lambda self: dec)
    monkeypatch.setattr(Config, "data_root", root)
    np.random.seed(0)
    ds = PosePC(train=False, vis=True, batch_length=20)
    assert ds.data_ti_.shape == (835, 20, 128, 6) and ds.data_ti_.dtype == np.float32
    assert ds.data_key_.shape == (835, 20, 21, 3) and ds.imu_.shape == (835, 20, 20, 15) and ds.skl_.shape == (835, 20, 3)
    assert np.array_equal(ds.data_ti_[sel], real["x"]), "padded point clouds must be bit-identical under the same seed"
    assert np.array_equal(ds.data_key_[sel].astype(np.float32), real["target"])
    assert np.array_equal(ds.skl_[sel].astype(np.float32), real["skl"])
    assert np.array_equal(ds.R_R0R_[sel].astype(np.float32), real["R"])
    assert np.array_equal(ds.imu_[sel].astype(np.float32), real["imu"])
    assert len(ds) == 835 and len(ds[0]) == 9
    b = next(batches(ds, 4, False))
    assert b[0].shape == (4, 20, 128, 6) and len(b) == 9
    # train/test split sizes of the seeded shuffle (80/20)
    np.random.seed(0)
    tr = PosePC(train=True, batch_length=20)
    assert len(tr) == int(835 * 0.8) and len(tr[0]) == 8
