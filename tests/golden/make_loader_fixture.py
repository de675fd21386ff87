#!/usr/bin/env python3
"""Generate tests/golden/g11_loader.npz: what tests/test_data_cpu.py needs, beside tests/golden/real16.npz, to check the
Sample_data loader without the data set itself (153 MB, 19 208 .mat files).

    python tests/golden/make_loader_fixture.py /path/to/Sample_data

Two parts, both plain data:
  * ``mat.*``: the first snippet the loader uses (01/04, 94 frames): the name of every frame file and its point count, the
    name of the snippet directory skipped in front of it, and the keys the loader reads from the frames that window 0 of
    real16.npz depends on -- the first frame (the rotation reference of the whole set) and the last 20 (the window).  The
    frames between them reach window 0 only through their point counts (numpy's RNG), so the test writes them with zeros.
  * ``dec.*``: the decoded layout of the WHOLE set -- points per frame, frames per snippet, the bone vectors.  With it the
    test rebuilds the decoded frames of the 16 windows of real16.npz from real16.npz itself and checks the loader's
    windows, its RNG draws over all 19 114 frames, the set size and the 80/20 split.
"""
import os
import sys

import numpy as np
import scipy.io as scio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from mmego_amd import data as md  # noqa: E402
from mmego_amd.config import Config  # noqa: E402

MAT_KEYS = ("pc_xyziv_ti2", "pc_xyz_key_2", "imu_save_l", "R_btc", "orientation_imu_img", "t_R0R", "abcd_ground_2", "foot_contact")
L = 20


def main(root):
    out = {}
    # ---- part 1: the first snippet in use; full frames: the first one and the last L
    snippets = md.list_snippets(root)
    a0, j0, files = snippets[0]
    action = sorted(os.listdir(root), key=lambda n: int(n))[a0]
    snips = sorted(os.listdir(os.path.join(root, action)))
    mats = [scio.loadmat(f) for f in files]
    full = [0] + list(range(len(files) - L, len(files)))
    out["mat.dirs"] = np.array([action, snips[0], snips[j0]])
    out["mat.names"] = np.array([os.path.basename(f) for f in files])
    out["mat.npts"] = np.array([m["pc_xyziv_ti2"].shape[0] for m in mats], dtype=np.int16)
    out["mat.full"] = np.array(full, dtype=np.int16)
    for k in MAT_KEYS:
        out["mat." + k] = np.concatenate([mats[i][k] for i in full], 0)
    # ---- part 2: the decoded layout of the whole set
    os.environ["MMEGO_CACHE_DIR"] = "off"
    ds = md.PosePC.__new__(md.PosePC)
    ds.root, ds.joint_selection, ds.skeleton = root, Config.kinect_joint_selection, Config.skeleton_all.tolist()
    dec = ds._decode()
    assert dec["npts"].max() < 2 ** 15
    out["dec.npts"] = dec["npts"].astype(np.int16)
    out["dec.snip_len"] = dec["snip_len"].astype(np.int16)
    out["dec.bones"] = dec["bones"]
    path = os.path.join(HERE, "g11_loader.npz")
    np.savez_compressed(path, **out)
    print("bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["MMEGO_DATA_ROOT"])
