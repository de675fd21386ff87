"""What the temporal filter of the blended rotations (dense.dense_infer(blend_space="rot", rot_smooth=(H, order, taper)): --infer
--dense --blend_space rot --rot_smooth H) costs and changes, in ONE process:

  python scripts/bench_dense_rot_smooth.py OUT.json

(a) device-event time of the two mmego_smooth_rot launches alone (J = 15 with 14 bones, moved, rot_moved and the fallback counts;
    J = 8 with 6 bones and the fallback counts) at F = 512 and 32 768 frames in segments of 64, H = 4, order 2, the gauss taper, on
    rigid rows whose rotations jitter by up to 0.6 rad a frame; beside them, as the yardstick, the two mmego_smooth_bones launches at
    the same F, H and order on the same rows (the nearest kernel before this option: 12 bytes per joint and tap where the rotation form
    reads 16 bytes per bone and tap, and no eigen-solve) -- the forms alternating, 20 chains of 10 calls after 3, a chain per event pair
    so that the timed window is not a single launch;
(b) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, about 19 100 frames; frame_no 20, window minibatch 64) at stride 5 under blend_space="rot": without the argument
    and with rot_smooth=(4, 2, "gauss") -- alternating, five rounds, medians, and the band of the rounds; and the host time of the
    two rot_jitter_deg figures of such a pass;
(c) what it changes, with the committed pretrained weights on the synthetic frames, --metrics full, stride 5: the displacement, the
    mean turn, the rotational jitter and the acceleration error before and after, for H = 2, 4, 8 and the three orders.  Random clouds
    and random targets: no error figure says anything about accuracy; the jitter figures show the mechanics only."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_dense_bones import chains_us, golden, load  # noqa: E402
from bench_frame_store import rounds, synthetic_frames  # noqa: E402
from mmego_amd import dense, hip, nets, ops, processors, skeleton  # noqa: E402
from mmego_amd.config import ConfigDemo  # noqa: E402
from mmego_amd.data import PosePC  # noqa: E402

dev = torch.device("cuda:0")
T, B, H, ORDER = 20, 64, 4, 2


def rigid_rows(rng, F, walk, body, J):
    """F rigid rows [F, 3 J] with their quaternions [F, NB, 4] (float32): a base rotation per bone times a rotation of at most 0.6 rad
    about a random axis in every frame, roots N(0, 0.7), vectorised."""
    NB = len(walk)

    def quats(n, angle):
        axis = rng.normal(size=(n, NB, 3))
        axis /= np.linalg.norm(axis, axis=2, keepdims=True)
        return np.concatenate([np.cos(angle / 2)[..., None], np.sin(angle / 2)[..., None] * axis], axis=2)

    def mul(a, b):
        w1, x1, y1, z1 = (a[..., i] for i in range(4))
        w2, x2, y2, z2 = (b[..., i] for i in range(4))
        return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)
    q = mul(quats(1, rng.uniform(0, np.pi, (1, NB))), quats(F, rng.uniform(-0.6, 0.6, (F, NB))))
    w, x, y, z = (q[..., i] for i in range(4))
    Q = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1).reshape(F, NB, 3, 3)
    pos = rng.normal(0.0, 0.7, (F, J, 3))
    for b, (c, p) in enumerate(walk.tolist()):
        pos[:, c] = pos[:, p] + Q[:, b] @ body[b].astype(np.float64)
    return pos.reshape(F, 3 * J).astype(np.float32), q.astype(np.float32)


def main(path):
    hip.lib()
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    up, lo = load(nets.UpperNet(), golden("w_upper_pretrained.npz")), load(nets.LowerNet(64), golden("w_lower_pretrained.npz"))
    res = {"shape": {"frame_no": T, "window_minibatch": B, "H": H, "order": ORDER, "taper": "gauss"},
           "method": "launches: device events around a chain of 10 calls, the forms alternating, 20 repetitions after 3, per call; passes: "
                     "wall clock around a whole pass (its last statement is a device -> host read), one warm pass each, then the passes "
                     "alternating, five rounds, medians"}

    # (a) the launches
    rng = np.random.default_rng(0)
    wd = torch.as_tensor(dense.smooth_weights(H, "gauss")).to(dev)
    res["launch_us"] = {}
    for F in (512, 32768):
        seg = torch.as_tensor((np.arange(F) // 64).astype(np.int32)).to(dev)
        forms, keep = {}, []
        for name, walk, J in (("upper", skeleton.WALK_UPPER, 15), ("lower", skeleton.WALK_LOWER, 8)):
            NB = len(walk)
            body = (0.25 * rng.normal(size=(NB, 3))).astype(np.float32)
            L = np.linalg.norm(body.astype(np.float64), axis=1).astype(np.float32)
            src_h, quat_h = rigid_rows(rng, F, walk, body, J)
            src, quat = torch.as_tensor(src_h).to(dev), torch.as_tensor(quat_h).to(dev)
            dst, qo = torch.empty((F, 3 * J), device=dev), torch.empty((F, NB, 4), device=dev)
            moved, rmoved = torch.empty(F, device=dev), torch.empty(F, device=dev)
            fell, fell_b = (torch.zeros(F, dtype=torch.int32, device=dev) for _ in range(2))
            bd, ld, _ = ops._bones_on(walk, L, J, dev, "bench")
            yd = torch.as_tensor(body).to(dev)
            first = name == "upper"                        # (the pass asks the upper launch for moved and rot_moved, the lower for neither)

            def add(name=name, J=J, NB=NB, src=src, quat=quat, dst=dst, qo=qo, moved=moved, rmoved=rmoved, fell=fell, fell_b=fell_b, bd=bd, ld=ld,
                    yd=yd, first=first):
                forms["smooth_rot %s (J = %d, %d bones)" % (name, J, NB)] = lambda: hip.call(
                    "smooth_rot", src, 3 * J, F, J, quat, NB, seg, wd, H, ORDER, bd, yd, dst, 3 * J, qo, moved if first else None,
                    rmoved if first else None, fell)
                forms["smooth_bones %s (J = %d, %d bones)" % (name, J, NB)] = lambda: hip.call(
                    "smooth_bones", src, 3 * J, F, J, seg, wd, H, ORDER, bd, ld, NB, dst, 3 * J, moved if first else None, fell_b)
            add()
            keep.append((src, quat, dst, qo, moved, rmoved, fell))
        t = chains_us(forms)
        both = lambda kind: sum(v["median"] for k, v in t.items() if k.startswith(kind))
        t["both smooth_rot launches"], t["both smooth_bones launches"] = round(both("smooth_rot"), 2), round(both("smooth_bones"), 2)
        t["smooth_rot / smooth_bones"] = round(both("smooth_rot") / both("smooth_bones"), 3)
        assert int(keep[0][6].sum()) == 0 and int(keep[1][6].sum()) == 0, "no fallback on these rows"
        res["launch_us"]["F = %d" % F] = t
    print("launch_us", res["launch_us"])

    # (b) the pass
    dec = synthetic_frames()
    PosePC._decode = lambda self: dec
    np.random.seed(0)
    ds = PosePC(train=False, vis=True, batch_length=T, root=os.path.join(ROOT, "scripts"), keep_frames=True)
    res["frames"] = int(len(ds.frame_npts_))

    def timed_pass(**more):
        def s():
            t0 = time.perf_counter()
            dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, blend_space="rot", **more)
            return time.perf_counter() - t0
        return s
    timers = {"stride 5, rot": timed_pass(), "stride 5, rot, rot_smooth": timed_pass(rot_smooth=(H, ORDER, "gauss"))}
    for t in timers.values():
        t()
    res["pass_s"] = rounds(timers, 5)
    base_s = res["pass_s"]["stride 5, rot"]
    res["pass_s"]["band of the rot rounds / median"] = round((max(base_s["rounds"]) - min(base_s["rounds"])) / base_s["median"], 4)
    res["pass_s"]["rot_smooth / rot"] = round(res["pass_s"]["stride 5, rot, rot_smooth"]["median"] / base_s["median"], 4)
    s, a = dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, blend_space="rot", rot_smooth=(H, ORDER, "gauss"))
    t0 = time.perf_counter()
    for k in ("rot", "rot_unsmoothed"):                    # (the two host figures of a pass, float64 numpy over the downloaded quaternions)
        dense.rot_jitter_deg(a[k], a["recording"], a["covered"])
    res["pass_s"]["rot_jitter_deg x 2 on the host inside a pass, ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print("pass_s", res["pass_s"])

    # (c) the effect
    res["effect_synthetic"] = {"note": "pretrained weights on random clouds against random targets: the figures show the mechanics, not accuracy"}
    keys = ("moved_cm", "rot_moved_deg", "rot_jitter_deg", "unsmoothed_rot_jitter_deg", "accel_cm", "unsmoothed_accel_cm", "all_cm",
            "unsmoothed_all_cm", "bone_dev_cm")
    for h in (2, 4, 8):
        for order in (0, 1, 2):
            s, _ = dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, metrics="full", blend_space="rot", rot_smooth=(h, order, "gauss"))
            res["effect_synthetic"]["H %d order %d gauss" % (h, order)] = dict({k: round(float(s[k]), 5) for k in keys},
                                                                            rot_smooth_fallback=s["rot_smooth_fallback"])
    print("effect_synthetic", res["effect_synthetic"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense_rot_smooth.json")
